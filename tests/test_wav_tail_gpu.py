"""The waveform tail on the GPU (tts_spec_to_mag, tts_deemphasis, tts_wav_finish; AudioProcessor's
inv_spectrogram_batch / deemphasis_batch / finish_batch; Synthesizer with ``wav_tail_device="gpu"``)
against the host path.

Yardsticks, as in tests/test_griffin_lim.py: the same formula evaluated in numpy float32 on the same
float32 inputs. The GPU's max-abs error against the float64 result may be at most ``FACTOR`` = 8 times
the float32 evaluation's; every figure is printed before it is asserted. The endpoints and the
16-bit samples have no tolerance: they equal the host's.
"""
import functools
import io
import json

import numpy as np
import pytest
import scipy.io.wavfile
import scipy.signal
import torch

from tts_amd.audio import AudioProcessor, wav_bytes

pytestmark = pytest.mark.gpu

FACTOR = 8.0
AUDIO = dict(fft_size=1024, win_length=1024, hop_length=256, sample_rate=22050, preemphasis=0.0, ref_level_db=20,
             power=1.5, griffin_lim_iters=30, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0, spec_gain=20,
             signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0, clip_norm=True)
PAD = 1e3  # what the padding of every input holds: a sample read past a row's length would show


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


def _put(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# -- 1. tts_spec_to_mag ------------------------------------------------------------------------

def _spec_expr(ap, x, dt):
    """`_db_to_amp(_denormalize(x)) ** power` on (n_freq, M) evaluated in dtype dt."""
    x = x.astype(dt)
    if ap.signal_norm:
        mx, lo, ref = dt(ap.max_norm), dt(ap.min_level_db), dt(ap.ref_level_db)
        if ap.symmetric_norm:
            if ap.clip_norm:
                x = np.clip(x, -mx, mx)
            x = (x + mx) * -lo / (dt(2) * mx) + lo + ref
        else:
            if ap.clip_norm:
                x = np.clip(x, dt(0), mx)
            x = x * -lo / mx + lo + ref
    return np.power(dt(10), x / dt(ap.spec_gain)) ** dt(ap.power)


@pytest.mark.parametrize("n_freq", [513, 1025])
@pytest.mark.parametrize("spec_gain", [1, 20])
@pytest.mark.parametrize("norm", ["symmetric_clip", "asymmetric_noclip", "none"])
def test_spec_to_mag_vs_numpy(norm, spec_gain, n_freq):
    """B = 3 ragged (7, 1, 12 frames). The level range follows the gain (dB at 20, log10 units at
    1), so that the magnitudes stay inside float32 at both; the inputs reach 25 % past the
    normalised range on both sides, so the clip works where it is on."""
    from tts_amd._lib import get_engine
    dev = _dev()
    span, ref_db = (100.0, 20.0) if spec_gain == 20 else (5.0, 1.0)
    kw = dict(spec_gain=spec_gain, fft_size=2 * (n_freq - 1), min_level_db=-span, ref_level_db=ref_db)
    kw.update({"symmetric_clip": {}, "asymmetric_noclip": {"symmetric_norm": False, "clip_norm": False},
               "none": {"signal_norm": False}}[norm])
    ap = AudioProcessor(**dict(AUDIO, **kw))
    lens, M = [7, 1, 12], 12
    rs = np.random.RandomState(7)
    if norm == "symmetric_clip":
        lo, hi = -1.25 * ap.max_norm, 1.25 * ap.max_norm
    elif norm == "asymmetric_noclip":
        lo, hi = -0.25 * ap.max_norm, 1.25 * ap.max_norm
    else:
        lo, hi = -span - 0.25 * span + ref_db, 0.25 * span + ref_db
    x = np.full((3, M, n_freq), PAD, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = rs.uniform(lo, hi, (n, n_freq))
    scale, offset, clip = ap._denorm_affine(n_freq)
    assert (clip is not None) == (norm == "symmetric_clip")
    S = torch.full((3, M, n_freq), float("nan"), device=dev)
    get_engine(dev).spec_to_mag(_put(x, dev), lens, _put(scale, dev), _put(offset, dev), clip, ap.spec_gain, ap.power,
                                S)
    S = S.cpu().numpy().astype(np.float64)
    assert np.isfinite(S).all()
    err = err32 = peak = 0.0
    for b, n in enumerate(lens):
        assert (S[b, n:] == 0).all(), b
        ref = ap._db_to_amp(ap._denormalize(x[b, :n].T.astype(np.float64))) ** ap.power
        assert np.abs(ref - _spec_expr(ap, x[b, :n].T, np.float64)).max() <= 1e-12 * ref.max()
        peak = max(peak, ref.max())
        err = max(err, np.abs(S[b, :n].T - ref).max())
        err32 = max(err32, np.abs(_spec_expr(ap, x[b, :n].T, np.float32).astype(np.float64) - ref).max())
    err, err32 = err / peak, err32 / peak
    print(f"spec_to_mag {norm} gain {spec_gain} n_freq {n_freq}: gpu {err:.3e} float32-numpy {err32:.3e} "
          f"ratio {err / err32:.2f}")
    assert err <= FACTOR * err32


def test_spec_to_mag_argument_errors():
    from tts_amd._lib import get_engine
    dev = _dev()
    eng = get_engine(dev)
    one = torch.ones(1026, device=dev)
    for n_freq, lens, gain, name in ((1026, [2], 20.0, "n_freq"), (513, [3], 20.0, "h_lens"),
                                     (513, [2], 0.0, "spec_gain")):
        S = torch.full((1, 2, n_freq), 7.0, device=dev)
        with pytest.raises(RuntimeError, match="spec_to_mag.*" + name):
            eng.spec_to_mag(torch.zeros(1, 2, n_freq, device=dev), lens, one, one, None, gain, 1.5, S)
        torch.cuda.synchronize()
        assert (S == 7.0).all()


# -- 2. tts_deemphasis -------------------------------------------------------------------------

DE_LENS = [1024, 1, 70001, 2, 1025, 1023]
DE_LMAX = 70010


@functools.lru_cache(maxsize=None)
def _deemph_input():
    """Noise on a DC offset: the offset drives the output towards 1 / (1 - a), the worst case."""
    rs = np.random.RandomState(0)
    x = np.full((len(DE_LENS), DE_LMAX), PAD, np.float32)
    for b, n in enumerate(DE_LENS):
        x[b, :n] = 0.3 * rs.randn(n) + 0.35
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _deemph_refs(a):
    """Per row: scipy's lfilter in float64 on the float32 samples, and the error of the sequential
    recurrence in numpy float32 with np.float32(a)."""
    x = _deemph_input()
    a32 = np.float32(a)
    out = []
    for b, n in enumerate(DE_LENS):
        ref = scipy.signal.lfilter([1], [1, -a], x[b, :n].astype(np.float64))
        y, prev = np.empty(n, np.float32), np.float32(0)
        for i in range(n):
            prev = x[b, i] + a32 * prev
            y[i] = prev
        assert y.dtype == np.float32 and prev.dtype == np.float32
        out.append((ref, np.abs(y.astype(np.float64) - ref).max()))
    return out


@pytest.mark.parametrize("a", [0.97, 0.98, 0.5])
def test_deemphasis_vs_lfilter(a):
    """One ragged, unsorted call; every row against lfilter within 8 x the float32 recurrence's
    error, bit for bit its own B = 1 call (on a tensor of its own length, so the partition cannot
    lean on L_max), zero past its length, and the same in place."""
    from tts_amd._lib import get_engine
    dev = _dev()
    eng = get_engine(dev)
    x = torch.from_numpy(_deemph_input().copy()).to(dev)
    out = torch.full_like(x, float("nan"))
    eng.deemphasis(x, DE_LENS, a, out)
    inplace = x.clone()
    eng.deemphasis(inplace, DE_LENS, a, inplace)
    assert torch.equal(inplace, out)
    y = out.cpu().numpy()
    for b, (n, (ref, err32)) in enumerate(zip(DE_LENS, _deemph_refs(a))):
        assert (y[b, n:] == 0).all(), b
        err = np.abs(y[b, :n].astype(np.float64) - ref).max()
        print(f"deemphasis a={a} n={n}: gpu {err:.3e} float32-numpy {err32:.3e} max|ref| {np.abs(ref).max():.2f}")
        assert err <= FACTOR * err32, (a, n, err, err32)
        single = torch.full((1, n), float("nan"), device=dev)
        eng.deemphasis(x[b:b + 1, :n].contiguous(), [n], a, single)
        assert torch.equal(single[0], out[b, :n]), (a, n)


def test_deemphasis_argument_errors():
    from tts_amd._lib import get_engine
    dev = _dev()
    eng = get_engine(dev)
    x = torch.zeros(1, 10, device=dev)
    for a, n, name in ((1.0, 10, "coefficient"), (0.0, 10, "coefficient"), (0.97, 11, "h_nsamples")):
        out = torch.full_like(x, 7.0)
        with pytest.raises(RuntimeError, match="deemphasis.*" + name):
            eng.deemphasis(x, [n], a, out)
        torch.cuda.synchronize()
        assert (out == 7.0).all()


# -- 3. endpoints and finish_batch -------------------------------------------------------------

def _tail_ap(sample_rate):
    return AudioProcessor(**dict(AUDIO, sample_rate=sample_rate))


@functools.lru_cache(maxsize=None)
def _rows(sample_rate):
    """Rows whose host endpoint is known by construction. window = int(0.8 sr), hop = int(window / 4);
    `loud` is noise that no window of is silent, `quiet` stays below half the threshold (0.01)."""
    window = int(sample_rate * 0.8)
    hop = int(window / 4)
    rs = np.random.RandomState(9)
    thr = np.float32(0.01)
    assert float(thr) < 0.01  # the float32 nearest the threshold lies below it

    def loud(n):
        return (0.2 * rs.randn(n)).astype(np.float32)

    def quiet(n):
        return rs.uniform(-0.005, 0.005, n).astype(np.float32)

    def with_sample(v):  # quiet from 20000 on, one sample v inside the first quiet windows
        w = np.concatenate([loud(20000), quiet(4 * window - 20000)])
        w[30000] = v
        return w

    first = hop * -(-20000 // hop)  # the first candidate window that starts in the quiet part
    negative = np.concatenate([loud(20000), quiet(3 * window)])
    negative[20000::100] = -0.5
    rows = {
        "short": (loud(window + hop - 5), window + hop - 5),
        "mid": (np.concatenate([loud(20000), quiet(3 * window)]), first + hop),
        "never": (loud(3 * window + 17), 3 * window + 17),
        "negative": (negative, first + hop),
        "thr_equal": (with_sample(thr), first + hop),
        "thr_below": (with_sample(np.nextafter(thr, np.float32(0))), first + hop),
        # a window holding the sample is alive: the first silent one starts after it
        "thr_above": (with_sample(np.nextafter(thr, np.float32(1))), hop * (30000 // hop + 1) + hop),
    }
    for w, _ in rows.values():
        w.setflags(write=False)
    return rows


def _host_tail(ap, rows, gap=10000):
    """Synthesizer.tts's host tail on float32 rows: endpoints and the int16 samples it writes."""
    ends, wavs = [], []
    for w in rows:
        end = ap.find_endpoint(w)
        ends.append(end)
        wavs += list(w[:end])
        wavs += [0] * gap
    sr, pcm = scipy.io.wavfile.read(io.BytesIO(wav_bytes(ap, np.asarray(wavs, np.float32)).getvalue()))
    assert sr == ap.sample_rate and pcm.dtype == np.int16
    return ends, pcm


def _check_finish(ap, rows):
    dev = _dev()
    L = max(len(w) for w in rows) + 13
    x = np.full((len(rows), L), PAD, np.float32)
    for b, w in enumerate(rows):
        x[b, :len(w)] = w
    pcm, ends = ap.finish_batch(torch.from_numpy(x).to(dev), [len(w) for w in rows])
    ref_ends, ref_pcm = _host_tail(ap, rows)
    print("endpoints", ends, "host", ref_ends, "samples", len(pcm))
    assert ends == ref_ends
    assert isinstance(pcm, np.ndarray) and pcm.dtype == np.int16
    assert np.array_equal(pcm, ref_pcm)
    return ends, pcm


@pytest.mark.parametrize("sample_rate", [22050, 22052])
def test_finish_batch_five_rows(sample_rate):
    ap, rows = _tail_ap(sample_rate), _rows(sample_rate)
    if sample_rate == 22052:
        assert int(sample_rate * 0.8) == 17641 and int(17641 / 4) == 4410  # the window is not four hops
    names = ["mid", "short", "thr_above", "never", "negative"]
    for n in names:  # the construction gives the host answer
        assert ap.find_endpoint(rows[n][0]) == rows[n][1], n
    ends, pcm = _check_finish(ap, [rows[n][0] for n in names])
    assert ends == [rows[n][1] for n in names]
    assert np.abs(pcm).max() >= 32766  # the peak sample times 32767 / peak, truncated


@pytest.mark.parametrize("sample_rate", [22050, 22052])
@pytest.mark.parametrize("name", ["thr_equal", "thr_below", "mid"])
def test_finish_batch_single_row(name, sample_rate):
    ap, (w, end) = _tail_ap(sample_rate), _rows(sample_rate)[name]
    assert ap.find_endpoint(w) == end
    assert _check_finish(ap, [w])[0] == [end]


@pytest.mark.parametrize("sample_rate", [22050, 22052])
def test_finish_batch_all_quiet(sample_rate):
    """Peak below 0.01: save_wav's factor is 32767 / 0.01, taken to float32."""
    ap = _tail_ap(sample_rate)
    rs = np.random.RandomState(12)
    rows = [rs.uniform(-0.004, 0.004, n).astype(np.float32) for n in (30000, 500)]
    hop = int(int(sample_rate * 0.8) / 4)
    ends, pcm = _check_finish(ap, rows)
    assert ends == [2 * hop, 500]
    assert 0 < np.abs(pcm).max() < 0.004 * 3276700.0 + 1


def test_wav_finish_argument_errors():
    from tts_amd._lib import get_engine
    dev = _dev()
    eng = get_engine(dev)
    x = torch.zeros(1, 100, device=dev)
    pcm = torch.full((200,), 7, dtype=torch.int16, device=dev)
    meta = torch.full((2,), 7, dtype=torch.int32, device=dev)
    for n, window, hop, gap, name in ((101, 40, 10, 5, "h_nsamples"), (100, 40, 0, 5, "hop_length"),
                                      (100, 5, 10, 5, "hop_length"), (100, 40, 10, -1, "gap")):
        with pytest.raises(RuntimeError, match="wav_finish.*" + name):
            eng.wav_finish(x, [n], window, hop, 0.01, gap, pcm, meta[:1], meta[1:])
    torch.cuda.synchronize()
    assert (pcm == 7).all() and (meta == 7).all()


# -- 4. inv_spectrogram_batch ------------------------------------------------------------------

GL_LENS = [24, 9, 30]


class _Rng:
    def __init__(self, u):
        self.u = u

    def rand(self, *shape):
        assert tuple(shape) == self.u.shape
        return self.u


@functools.lru_cache(maxsize=None)
def _gl_inputs():
    """Normalised linear spectrograms (513, M) of three chirps and their phase numbers (float32
    values, so that the CPU and the GPU see the same)."""
    cpu = AudioProcessor(**AUDIO)
    specs, phases = [], []
    for i, M in enumerate(GL_LENS):
        t = np.arange(256 * (M - 1)) / 22050.0
        wav = 0.3 * np.sin(2 * np.pi * (220.0 + 40 * i) * t) + 0.2 * np.sin(2 * np.pi * (500.0 + 900.0 * t) * t)
        spec = cpu.spectrogram(wav)
        assert spec.shape == (513, M)
        specs.append(spec)
        phases.append(np.random.RandomState(3 + i).rand(513, M).astype(np.float32).astype(np.float64))
    return cpu, specs, phases


def _gl_batch(ap, specs, phases, rows, **kw):
    dev = _dev()
    lens = [specs[b].shape[1] for b in rows]
    x = np.full((len(rows), max(lens), 513), PAD, np.float32)
    u = np.full((len(rows), max(lens), 513), PAD, np.float32)
    for j, b in enumerate(rows):
        x[j, :lens[j]] = specs[b].T
        u[j, :lens[j]] = phases[b].T
    wav, counts = ap.inv_spectrogram_batch(torch.from_numpy(x).to(dev), lens, torch.from_numpy(u).to(dev), **kw)
    assert wav.shape == (len(rows), 256 * (max(lens) - 1)) and counts == [256 * (n - 1) for n in lens]
    return wav, counts


def test_inv_spectrogram_batch_vs_cpu():
    cpu, specs, phases = _gl_inputs()
    gpu = AudioProcessor(**dict(AUDIO, griffin_lim_device="gpu"))
    wav, counts = _gl_batch(gpu, specs, phases, [0, 1, 2])
    y = wav.cpu().numpy()
    assert np.isfinite(y).all()
    for b, n in enumerate(counts):
        ref = cpu.inv_spectrogram(specs[b], _Rng(phases[b]))
        assert ref.shape == (n,) and (y[b, n:] == 0).all()
        S = cpu._db_to_amp(cpu._denormalize(specs[b])) ** cpu.power  # the magnitudes Griffin-Lim is given

        def conv(w):
            return np.linalg.norm(np.abs(cpu._stft(w)) - S) / np.linalg.norm(S)

        sc_gpu, sc_cpu = conv(y[b, :n].astype(np.float64)), conv(ref)
        print(f"row {b} M={GL_LENS[b]} spectral convergence: gpu {sc_gpu:.6e} cpu {sc_cpu:.6e}")
        assert abs(sc_gpu - sc_cpu) <= 1e-3 * sc_cpu
        single, _ = _gl_batch(gpu, specs, phases, [b])
        assert torch.equal(single[0], wav[b, :n]), b


def test_inv_spectrogram_batch_deemphasis_on_the_device():
    _, specs, phases = _gl_inputs()
    gpu = AudioProcessor(**dict(AUDIO, griffin_lim_iters=4, preemphasis=0.97, griffin_lim_device="gpu"))
    raw, counts = _gl_batch(gpu, specs, phases, [0, 1, 2], deemphasis=False)
    done, _ = _gl_batch(gpu, specs, phases, [0, 1, 2])
    assert not torch.equal(done, raw)
    assert torch.equal(done, gpu.deemphasis_batch(raw, counts))
    plain = AudioProcessor(**dict(AUDIO, griffin_lim_iters=4, griffin_lim_device="gpu"))
    assert torch.equal(_gl_batch(plain, specs, phases, [0, 1, 2])[0], raw)


def test_inv_spectrogram_batch_refuses_what_the_host_refuses(tmp_path):
    """Mean-var stats and 513 bins: `_scaler_for` compares with fft_size / 2 as the reference does,
    so the host path raises, and so does the batch."""
    dev = _dev()
    rs = np.random.RandomState(11)
    st = {"mel_mean": rs.uniform(-3, -1, 80), "mel_std": rs.uniform(0.3, 0.8, 80),
          "linear_mean": rs.uniform(-3, -1, 513), "linear_std": rs.uniform(0.3, 0.8, 513)}
    acfg = {k: v for k, v in AUDIO.items() if k not in ("max_norm", "min_level_db", "symmetric_norm", "clip_norm")}
    acfg["stats_path"] = str(tmp_path / "scale_stats.npy")
    st["audio_config"] = acfg
    np.save(tmp_path / "scale_stats.npy", st, allow_pickle=True)
    ap = AudioProcessor(**dict(AUDIO, stats_path=acfg["stats_path"], griffin_lim_device="gpu"))
    with pytest.raises(RuntimeError, match="Mean-Var stats"):
        ap.inv_spectrogram(np.zeros((513, 12)))
    with pytest.raises(RuntimeError, match="Mean-Var stats"):
        ap.inv_spectrogram_batch(torch.zeros(1, 12, 513, device=dev), [12])


# -- 5. end to end -----------------------------------------------------------------------------

SENTENCES = "Hello world. This is a longer test of the batched path, with 2 numbers! Short one?"


def test_synthesizer_tts_bytes_equal_the_host_tail(tmp_path, capsys):
    """Tacotron2 + MB-MelGAN (deterministic): tts() with "wav_tail_device": "gpu" returns the bytes
    the host tail returns, and prints what it prints."""
    from test_gpu_parity import _synth_files
    from tts_amd.synthesizer import Synthesizer
    _dev()
    conf = _synth_files(tmp_path)
    out = {}
    for key in (None, "gpu"):
        for name in ("tts.json", "voc.json"):
            c = json.loads((tmp_path / name).read_text())
            c["audio"].pop("wav_tail_device", None)
            if key:
                c["audio"]["wav_tail_device"] = key
            (tmp_path / name).write_text(json.dumps(c))
        synth = Synthesizer(conf)
        assert synth.ap.wav_tail_device == key
        synth.tts_model.decoder.max_decoder_steps = 24
        capsys.readouterr()
        out[key] = synth.tts(SENTENCES).getvalue()
        printed = capsys.readouterr().out
        assert " > Processing time: " in printed and " > Real-time factor: " in printed
    sr, pcm = scipy.io.wavfile.read(io.BytesIO(out["gpu"]))
    assert sr == 22050 and pcm.dtype == np.int16 and len(pcm) == 3 * (24 * 2 * 256 + 10000)
    assert out["gpu"] == out[None]


def test_tacotron1_synthesizer_on_the_device(tmp_path):
    """Tacotron (v1) with both GPU keys and pre-emphasis 0.97: one inv_spectrogram_batch call on the
    postnet tensor, de-emphasis and the tail on the device. The phases are random, so the check is
    the shape of the result: a 22050 Hz int16 wav as long as the endpoints plus the gaps."""
    from tts_amd.spec import TacotronV1Config, tacotron_spec
    from tts_amd.synthesizer import Synthesizer
    from tts_amd.text import symbols
    from tts_amd.weights import synth_state_dict
    _dev()
    cfg = TacotronV1Config(num_chars=len(symbols), r=5, postnet_output_dim=513)
    sd = synth_state_dict(tacotron_spec(cfg), 31, {})
    sd["decoder.stopnet.linear.bias"] = np.array([-1e4], np.float32)  # runs to max_decoder_steps
    audio = dict(AUDIO, griffin_lim_iters=4, preemphasis=0.97, griffin_lim_device="gpu", wav_tail_device="gpu")
    tcfg = {"model": "Tacotron", "r": 5, "use_phonemes": False, "text_cleaner": "english_cleaners", "audio": audio,
            "memory_size": 5, "attention_norm": "sigmoid", "prenet_dropout": False, "separate_stopnet": True,
            "location_attn": True}
    (tmp_path / "tts.json").write_text(json.dumps(tcfg))
    torch.save({"model": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "r": 5},
               str(tmp_path / "tts.pth"))
    synth = Synthesizer({"use_cuda": True, "tts_checkpoint": str(tmp_path / "tts.pth"),
                         "tts_config": str(tmp_path / "tts.json"), "tts_speakers": None, "vocoder_checkpoint": None,
                         "vocoder_config": None, "wavernn_lib_path": None})
    synth.tts_model.decoder.max_decoder_steps = 6
    calls = []
    batch, finish = synth.ap.inv_spectrogram_batch, synth.ap.finish_batch

    def spy_batch(specs, lengths, *a, **kw):
        calls.append(("batch", tuple(specs.shape), specs.device.type))
        return batch(specs, lengths, *a, **kw)

    def spy_finish(wav, counts, *a, **kw):
        res = finish(wav, counts, *a, **kw)
        calls.append(("finish", list(counts), res[1]))
        return res

    synth.ap.inv_spectrogram_batch, synth.ap.finish_batch = spy_batch, spy_finish
    buf = synth.tts("Griffin and Lim. Phase from noise.")
    assert [c[0] for c in calls] == ["batch", "finish"]
    frames = int(synth.tts_model.last_mel_lengths[0])
    assert calls[0][1:] == ((2, frames, 513), "cuda")
    counts, ends = calls[1][1:]
    assert counts == [256 * (frames - 1)] * 2 and all(0 < e <= n for e, n in zip(ends, counts))
    sr, pcm = scipy.io.wavfile.read(io.BytesIO(buf.getvalue()))
    assert sr == 22050 and pcm.dtype == np.int16
    assert len(pcm) == sum(ends) + 2 * 10000 and np.abs(pcm).max() > 0
    # synthesize_batch hands the same rows to the host
    wavs = synth.synthesize_batch(["Griffin and Lim.", "Phase from noise."])
    assert [w.shape for w in wavs] == [(n,) for n in counts] and all(w.dtype == np.float32 for w in wavs)
