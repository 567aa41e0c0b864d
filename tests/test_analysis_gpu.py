"""Batched audio analysis on the GPU (tts_stft_mag, tts_mag_to_feature, AudioProcessor's
``analysis_device="gpu"``, SpeakerEncoder.embed_utterances) against the CPU path in float64.

Yardstick, as in tests/test_griffin_lim.py: truth is the float64 CPU path (AudioProcessor._stft,
melspectrogram, spectrogram); the GPU's error may be at most ``FACTOR`` = 8 times the error of the same
algorithm run in float32 on the CPU on the same input: torch.stft on float32 tensors for the FFT
kernel, a float32 matrix DFT over the double-computed twiddle table for the direct kernel, the numpy
feature expression in float32 for the feature step. Magnitude errors are max-abs per frame relative
to that frame's float64 peak, feature errors max-abs. Inputs are the chirp of test_griffin_lim.py's
``_speech``, rounded to float32 so that all three runs see the same samples. Every figure is printed
before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import build_taco, taco_state_dict
from tts_amd.audio import AudioProcessor

pytestmark = pytest.mark.gpu

FACTOR = 8.0
LJ_AUDIO = dict(fft_size=1024, win_length=1024, hop_length=256, sample_rate=22050, preemphasis=0.0,
                ref_level_db=20, power=1.5, griffin_lim_iters=30, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0,
                spec_gain=1, signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0,
                clip_norm=True)
LJ_PRE = dict(LJ_AUDIO, preemphasis=0.97, spec_gain=20)
# TTS/speaker_encoder/config.json
GE2E_AUDIO = dict(LJ_AUDIO, fft_size=400, win_length=400, hop_length=160, sample_rate=16000, preemphasis=0.98,
                  num_mels=40, mel_fmin=0.0, mel_fmax=8000.0, spec_gain=20)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


def _engine(dev):
    from tts_amd._lib import get_engine
    return get_engine(dev)


def _key(audio):
    return tuple(sorted(audio.items()))


def _speech(sr, n):
    t = np.arange(n) / sr
    y = 0.3 * np.sin(2 * np.pi * (200 + 300 * t) * t) + 0.05 * np.random.RandomState(3).randn(n)
    return y.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------ the float32 CPU yardsticks
def _preemph32(ap, y):
    y = y.astype(np.float32)
    if ap.preemphasis != 0:
        y = y - np.float32(ap.preemphasis) * np.concatenate([np.zeros(1, np.float32), y[:-1]])
    assert y.dtype == np.float32
    return y


def _mag_fft32(ap, y):
    """abs(torch.stft) on float32 tensors, (F, M)."""
    D = torch.stft(torch.from_numpy(_preemph32(ap, y)), ap.fft_size, ap.hop_length, ap.win_length,
                   ap._window().float(), center=True, pad_mode="reflect", return_complex=True)
    return np.abs(D.numpy()).astype(np.float64)


def _mag_dft32(ap, y):
    """A float32 matrix DFT of the windowed frames; the cos / sin table is computed in double, indexed
    by (k n) mod n_fft and cast to float32."""
    N, hop, wl = ap.fft_size, ap.hop_length, ap.win_length
    yp = np.pad(_preemph32(ap, y), N // 2, mode="reflect")
    win = np.zeros(N)
    win[(N - wl) // 2:(N - wl) // 2 + wl] = ap._window().numpy()
    fr = np.stack([yp[t * hop:t * hop + N] * win.astype(np.float32) for t in range(1 + len(y) // hop)])
    m = np.arange(N)
    idx = (np.arange(N // 2 + 1)[:, None] * m[None, :]) % N
    c, s = np.cos(-2 * np.pi * m / N).astype(np.float32), np.sin(-2 * np.pi * m / N).astype(np.float32)
    re, im = fr @ c[idx].T, fr @ s[idx].T
    assert re.dtype == np.float32
    return np.sqrt(re * re + im * im).T.astype(np.float64)


def _affine64(ap, mel):
    """(scale, offset, clip) of the feature step; with mean-var stats the linear scaler is taken
    directly (AudioProcessor._norm_affine keeps the reference's refusal of 513 channels)."""
    if hasattr(ap, "mel_scaler") and not mel:
        std, mean = np.asarray(ap.linear_scaler.scale_), np.asarray(ap.linear_scaler.mean_)
        return 1.0 / std, -mean / std, None
    return ap._norm_affine(ap.num_mels if mel else ap.fft_size // 2 + 1)


def _feature_expr(ap, mag, mel, dt):
    """_normalize(_amp_to_db(mel_basis @ mag)) (or of mag itself) on (F, M), evaluated in dtype dt."""
    X = mag.astype(dt)
    if mel:
        X = ap.mel_basis.astype(dt) @ X
    S = dt(ap.spec_gain) * np.log10(np.maximum(dt(1e-5), X))
    if not ap.signal_norm:
        return S
    if hasattr(ap, "mel_scaler"):
        sc = ap.mel_scaler if mel else ap.linear_scaler
        return ((S.T - sc.mean_.astype(dt)) / sc.scale_.astype(dt)).T
    mx, lo, ref = dt(ap.max_norm), dt(ap.min_level_db), dt(ap.ref_level_db)
    Sn = ((S - ref) - lo) / -lo
    if ap.symmetric_norm:
        Sn = (dt(2) * mx) * Sn - mx
        return np.clip(Sn, -mx, mx) if ap.clip_norm else Sn
    Sn = mx * Sn
    return np.clip(Sn, dt(0), mx) if ap.clip_norm else Sn


def _at_clip(ap, x):
    """Share of values sitting on a clip bound (clipping hides errors)."""
    if not (ap.signal_norm and ap.clip_norm) or hasattr(ap, "mel_scaler"):
        return 0.0
    lo = -ap.max_norm if ap.symmetric_norm else 0.0
    return float(np.mean((x <= lo) | (x >= ap.max_norm)))


@functools.lru_cache(maxsize=None)
def _case(audio_key, n, direct):
    """Input, float64 magnitudes and the float32-CPU magnitude error of one configuration."""
    ap = AudioProcessor(**dict(audio_key))
    y = _speech(ap.sample_rate, n)
    ref = np.abs(ap._preemph_stft(y))
    assert ref.shape == (ap.fft_size // 2 + 1, 1 + n // ap.hop_length)
    peak = ref.max(axis=0)
    m32 = (_mag_dft32 if direct else _mag_fft32)(ap, y)
    err32 = (np.abs(m32 - ref).max(axis=0) / peak).max()
    return dict(ap=ap, y=y, ref=ref, peak=peak, m32=m32, err32=err32)


def _gpu_mag(ap, rows, algo=0, out=None, M_max=None, fill=float("nan")):
    """tts_stft_mag on the waveform rows; the input holds NaN past each row's length."""
    dev = _dev()
    lens = [len(r) for r in rows]
    wav = np.full((len(rows), max(lens)), np.nan, np.float32)
    for b, r in enumerate(rows):
        wav[b, :len(r)] = r
    M = M_max or max(1 + n // ap.hop_length for n in lens)
    if out is None:
        out = torch.full((len(rows), M, ap.fft_size // 2 + 1), fill, device=dev)
    _engine(dev).stft_mag(torch.from_numpy(wav).to(dev), lens, ap.fft_size, ap.win_length, ap.hop_length,
                          ap.preemphasis, out, algo=algo)
    return out.cpu().numpy()


def _check_mag(name, mag, c):
    """mag (M, F) against the float64 magnitudes of the case."""
    assert mag.shape == c["ref"].T.shape, (mag.shape, c["ref"].shape)
    assert np.isfinite(mag).all()
    err = (np.abs(mag.astype(np.float64).T - c["ref"]).max(axis=0) / c["peak"]).max()
    print(f"{name}: gpu {err:.3e} float32-cpu {c['err32']:.3e} ratio {err / c['err32']:.2f}")
    assert err <= FACTOR * c["err32"], (name, err, c["err32"])


# ------------------------------------------------------------------------------ 1-3: magnitudes
@pytest.mark.parametrize("pre", [0.0, 0.97])
@pytest.mark.parametrize("n", [513, 768, 256 * 39 + 17])
def test_stft_fft_kernel_vs_cpu(n, pre):
    """Case 1: the FFT kernel at 1024 / 1024 / 256, B = 1. 513 samples is the shortest legal row (3
    frames, every one touching both reflect pads); 256 * 39 + 17 is no multiple of the hop."""
    audio = dict(LJ_AUDIO, preemphasis=pre)
    c = _case(_key(audio), n, False)
    mag = _gpu_mag(c["ap"], [c["y"]])[0]
    assert mag.shape[0] == 1 + n // 256
    _check_mag(f"stft fft 1024/1024/256 n={n} pre={pre}", mag, c)


@pytest.mark.parametrize("n", [513, 200 * 39 + 3])
def test_stft_short_window_odd_hop(n):
    """Case 2: window shorter than the FFT, hop that does not divide it."""
    c = _case(_key(dict(LJ_AUDIO, win_length=800, hop_length=200)), n, False)
    mag = _gpu_mag(c["ap"], [c["y"]])[0]
    assert mag.shape[0] == 1 + n // 200
    _check_mag(f"stft fft 1024/800/200 n={n}", mag, c)


@pytest.mark.parametrize("audio,n,algo", [(GE2E_AUDIO, 201, 0), (GE2E_AUDIO, 160 * 39 + 5, 0), (LJ_AUDIO, 768, 2)])
def test_stft_direct_kernel_vs_cpu(audio, n, algo):
    """Case 3: the direct DFT kernel at the GE2E parameters (400 / 400 / 160, pre-emphasis 0.98; 201
    samples is the shortest legal row) and, forced with algo = 2, at 1024 / 1024 / 256."""
    c = _case(_key(audio), n, True)
    ap = c["ap"]
    mag = _gpu_mag(ap, [c["y"]], algo=algo)[0]
    assert mag.shape[0] == 1 + n // ap.hop_length
    _check_mag(f"stft direct {ap.fft_size}/{ap.win_length}/{ap.hop_length} n={n}", mag, c)


def test_stft_ragged_batch():
    """Case 4: sample counts (513, 256 * 39 + 17, 1300) in one call. The input holds NaN past each
    row's length and the output was filled with NaN by a full-length NaN call of the same shape: every
    row is bit for bit its own B = 1 call (another L_max and M_max) and exactly zero past its frames."""
    ns = [513, 256 * 39 + 17, 1300]
    cs = [_case(_key(LJ_AUDIO), n, False) for n in ns]
    ap = cs[0]["ap"]
    dev = _dev()
    out = torch.zeros(3, 40, 513, device=dev)
    poisoned = _gpu_mag(ap, [np.full(max(ns), np.nan)] * 3, out=out)
    assert np.isnan(poisoned).all()
    mag = _gpu_mag(ap, [c["y"] for c in cs], out=out)
    assert mag.shape == (3, 40, 513)
    for b, (n, c) in enumerate(zip(ns, cs)):
        M = 1 + n // 256
        single = _gpu_mag(ap, [c["y"]])[0]
        assert single.shape == (M, 513)
        assert np.array_equal(mag[b, :M], single), b
        assert (mag[b, M:] == 0).all(), b
        _check_mag(f"ragged row {b} n={n}", mag[b, :M], c)


# ------------------------------------------------------------------------------ 5: feature step
def _norm_ap(norm, tmp_path, base=LJ_PRE):
    kw = {"symmetric": {}, "asymmetric": {"symmetric_norm": False}, "none": {"signal_norm": False}}.get(norm)
    if kw is None:  # a stats file as TTS/bin/compute_statistics.py writes it, dB-sized stats
        rs = np.random.RandomState(11)
        st = {"mel_mean": rs.uniform(-60, -20, 80), "mel_std": rs.uniform(6, 16, 80),
              "linear_mean": rs.uniform(-60, -20, 513), "linear_std": rs.uniform(6, 16, 513)}
        acfg = {k: v for k, v in base.items() if k not in ("max_norm", "min_level_db", "symmetric_norm",
                                                            "clip_norm")}
        acfg["stats_path"] = str(tmp_path / "scale_stats.npy")
        st["audio_config"] = acfg
        np.save(tmp_path / "scale_stats.npy", st, allow_pickle=True)
        kw = {"stats_path": acfg["stats_path"]}
    return AudioProcessor(**dict(base, **kw))


def _gpu_feature(ap, mags, lens, mel, fill=float("nan")):
    """tts_mag_to_feature on mags (B, M, F) float32."""
    dev = _dev()
    scale, offset, clip = _affine64(ap, mel)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    out = torch.full((mags.shape[0], mags.shape[1], scale.shape[0]), fill, device=dev)
    _engine(dev).mag_to_feature(put(mags), lens, put(ap.mel_basis) if mel else None, ap.spec_gain, put(scale),
                                put(offset), clip, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("norm", ["symmetric", "asymmetric", "none", "meanvar"])
@pytest.mark.parametrize("mel", [True, False])
def test_mag_to_feature_vs_numpy(mel, norm, tmp_path):
    """Case 5: mel (80) and linear (513) features in the four normalisations, lens [40, 25], against
    the numpy expression in float64; at most 8 x the same expression's float32 error; rows zero past
    their length."""
    ap = _norm_ap(norm, tmp_path)
    c = _case(_key(LJ_PRE), 256 * 39, False)
    mag = c["ref"].astype(np.float32)  # (513, 40): the same float32 magnitudes for all three
    ref = _feature_expr(ap, mag, mel, np.float64)
    if not (norm == "meanvar" and not mel):
        own = ap._normalize(ap._amp_to_db((ap.mel_basis @ mag.astype(np.float64)) if mel else mag.astype(np.float64)))
        assert np.abs(own - ref).max() <= 1e-12 * np.abs(ref).max()
    clipped = _at_clip(ap, ref)
    err32 = np.abs(_feature_expr(ap, mag, mel, np.float32) - ref).max()
    out = _gpu_feature(ap, np.stack([mag.T, mag.T]), [40, 25], mel)
    assert out.shape == (2, 40, 80 if mel else 513)
    assert np.isfinite(out).all() and (out[1, 25:] == 0).all()
    assert np.array_equal(out[1, :25], out[0, :25])
    err = np.abs(out[0].T.astype(np.float64) - ref).max()
    print(f"mag_to_feature {'mel' if mel else 'linear'} {norm}: gpu {err:.3e} float32-numpy {err32:.3e} "
          f"ratio {err / err32:.2f} at clip bound {clipped:.4%}")
    assert clipped < 0.01
    assert err <= FACTOR * err32


@pytest.mark.parametrize("mel", [True, False])
def test_mag_to_feature_clipping(mel):
    """Deliberate clipping (symmetric, clip_norm): an all-zero magnitude row sits on the 1e-5 floor,
    which is exactly -max_norm after clipping; a row scaled by 1e3 is exactly +max_norm wherever the
    float64 result clips."""
    ap = AudioProcessor(**LJ_PRE)
    c = _case(_key(LJ_PRE), 256 * 39, False)
    mag = c["ref"].astype(np.float32)
    loud = mag * np.float32(1e3)
    ref = _feature_expr(ap, loud, mel, np.float64)
    out = _gpu_feature(ap, np.stack([np.zeros_like(mag.T), loud.T]), [40, 40], mel)
    assert (out[0] == -ap.max_norm).all()
    top = ref.T >= ap.max_norm
    print(f"clipping {'mel' if mel else 'linear'}: {top.mean():.2%} of the loud row at +max_norm")
    assert top.mean() > 0.05
    assert (out[1][top] == ap.max_norm).all()
    assert (out[1] <= ap.max_norm).all() and (out[1] >= -ap.max_norm).all()


# ------------------------------------------------------------------------------ 6: the processor
@pytest.mark.parametrize("audio", [LJ_AUDIO, LJ_PRE], ids=["lj", "lj_pre"])
def test_processor_on_gpu_vs_cpu(audio):
    """Case 6: AudioProcessor(analysis_device="gpu").melspectrogram / .spectrogram against the CPU
    processor on the same samples: shape (C, M), error within 8 x that of the float32 CPU chain
    (float32 torch.stft, then the float32 feature expression)."""
    _dev()
    c = _case(_key(audio), 256 * 39, False)
    cpu, gpu = c["ap"], AudioProcessor(**audio, analysis_device="gpu")
    for mel, fn in ((True, "melspectrogram"), (False, "spectrogram")):
        ref = getattr(cpu, fn)(c["y"])
        err32 = np.abs(_feature_expr(cpu, c["m32"].astype(np.float32), mel, np.float32) - ref).max()
        clipped = _at_clip(cpu, ref)
        out = getattr(gpu, fn)(c["y"])
        assert isinstance(out, np.ndarray) and out.shape == ref.shape == (80 if mel else 513, 40)
        err = np.abs(out.astype(np.float64) - ref).max()
        print(f"processor {fn}: gpu {err:.3e} float32-cpu {err32:.3e} ratio {err / err32:.2f} "
              f"at clip bound {clipped:.4%}")
        assert clipped < 0.01
        assert np.isfinite(out).all() and err <= FACTOR * err32, fn


def test_melspectrogram_batch_rows_equal_single_calls():
    """Case 6, batch: two rows of different length in one melspectrogram_batch call equal their own
    B = 1 results bit for bit, and are zero past their frame counts."""
    dev = _dev()
    ap = AudioProcessor(**LJ_PRE, analysis_device="gpu")
    ns = [256 * 39, 1300]
    ys = [_speech(ap.sample_rate, n) for n in ns]
    wav = np.zeros((2, max(ns)), np.float32)
    for b, y in enumerate(ys):
        wav[b, :len(y)] = y
    out, frames = ap.melspectrogram_batch(torch.from_numpy(wav).to(dev), ns)
    assert frames == [40, 6] and out.shape == (2, 40, 80) and out.device.type == "cuda"
    out = out.cpu().numpy()
    for b, y in enumerate(ys):
        single = ap.melspectrogram(y)
        assert single.shape == (80, frames[b])
        assert np.array_equal(out[b, :frames[b]].T, single), b
        assert (out[b, frames[b]:] == 0).all(), b


# ------------------------------------------------------------------------------ 7: speaker path
def test_embed_utterances_vs_oracle_and_into_tacotron2():
    """Case 7: wav -> mel -> GE2E embedding on the device for two utterances of 171 and 96 frames
    (three windows with a ragged last one, and two) against the numpy oracle fed the float64 CPU mel.
    Bound 8 x (a + b): a = the oracle's own shift when fed the float32-CPU mel, b = the error of the
    existing GPU compute_embedding on the float64 mel. The embeddings then condition a Tacotron2."""
    from oracle.ge2e_np import Ge2eOracle
    from tts_amd import SpeakerEncoder
    from tts_amd.spec import Ge2eConfig, TacotronConfig, ge2e_spec
    from tts_amd.weights import synth_state_dict
    dev = _dev()
    sd = synth_state_dict(ge2e_spec(Ge2eConfig()), 12)
    m = SpeakerEncoder(40, 256, 768, 3, True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    go = Ge2eOracle(sd)
    cpu, gpu = AudioProcessor(**GE2E_AUDIO), AudioProcessor(**GE2E_AUDIO, analysis_device="gpu")
    ns = [160 * 170, 160 * 95 + 7]
    ys = [_speech(16000, n) for n in ns]
    wav = np.zeros((2, max(ns)), np.float32)
    for b, y in enumerate(ys):
        wav[b, :len(y)] = y
    emb = m.embed_utterances(torch.from_numpy(wav).to(dev), ns, gpu)
    assert emb.shape == (2, 256) and emb.device.type == "cuda"
    e = emb.cpu().numpy()
    a = b_ = err = 0.0
    for i, (y, T) in enumerate(zip(ys, [171, 96])):
        mel64 = cpu.melspectrogram(y)
        assert mel64.shape == (40, T)
        assert len(SpeakerEncoder.embedding_windows(T)) == (3 if i == 0 else 2)
        ref = go.compute_embedding(mel64.T)
        mel32 = _feature_expr(cpu, _mag_dft32(cpu, y).astype(np.float32), True, np.float32)
        a = max(a, float(np.abs(go.compute_embedding(mel32.T) - ref).max()))
        old = m.compute_embedding(torch.from_numpy(mel64.T.astype(np.float32)).to(dev)).cpu().numpy()[0]
        b_ = max(b_, float(np.abs(old - ref).max()))
        err = max(err, float(np.abs(e[i] - ref).max()))
    print(f"embed_utterances: gpu {err:.3e} oracle shift on float32 mel (a) {a:.3e} "
          f"gpu compute_embedding on float64 mel (b) {b_:.3e} ratio {err / (a + b_):.2f}")
    assert np.isfinite(e).all()
    assert err <= FACTOR * (a + b_)

    cfg = TacotronConfig(num_speakers=2, speaker_embedding_dim=256)
    _, tsd = taco_state_dict(None, seed=31, overrides={}, stop_bias=-1e4, cfg=cfg)
    taco = build_taco(cfg, tsd)
    taco.decoder.set_r(2)
    ids = np.random.RandomState(0).randint(1, 129, size=(2, 13)).astype(np.int64)
    ids[1, 9:] = 0
    ids = torch.from_numpy(ids).to(dev)
    _, post, _, _ = taco.inference(ids, text_lengths=[13, 9], max_decoder_steps=6, speaker_embeddings=emb)
    copied = torch.from_numpy(e).cuda()  # the existing way: a host array copied in
    _, post2, _, _ = taco.inference(ids, text_lengths=[13, 9], max_decoder_steps=6, speaker_embeddings=copied)
    post, post2 = post.cpu().numpy(), post2.cpu().numpy()
    assert post.shape == (2, 12, 80) and np.isfinite(post).all()
    assert np.array_equal(post, post2)


# ------------------------------------------------------------------------------ 8: argument errors
@pytest.mark.parametrize("bad", ["odd_n_fft", "short_row", "batch_65"])
def test_stft_argument_errors(bad):
    """Case 8: unsupported geometry is an error naming the entry point and leaves the output untouched."""
    dev = _dev()
    n_fft, rows = 1024, [2048, 2048]
    if bad == "odd_n_fft":
        n_fft = 1023
    elif bad == "short_row":  # no room for the reflect pad
        rows = [2048, 512]
    else:
        rows = [2048] * 65
    wav = torch.zeros(len(rows), 2048, device=dev)
    out = torch.full((len(rows), 9, 513), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="stft_mag") as e:
        _engine(dev).stft_mag(wav, rows, n_fft, 400, 256, 0.0, out)
    print(e.value)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_mag_to_feature_argument_errors():
    dev = _dev()
    mag = torch.zeros(65, 8, 513, device=dev)
    out = torch.full((65, 8, 513), 7.0, device=dev)
    one = torch.ones(513, device=dev)
    with pytest.raises(RuntimeError, match="mag_to_feature") as e:
        _engine(dev).mag_to_feature(mag, [8] * 65, None, 20.0, one, one, None, out)
    print(e.value)
    with pytest.raises(RuntimeError, match="mag_to_feature"):  # no basis, yet another channel count
        _engine(dev).mag_to_feature(mag[:2], [8, 8], None, 20.0, one, one, None, out[:2, :, :80].contiguous())
    torch.cuda.synchronize()
    assert (out == 7.0).all()
