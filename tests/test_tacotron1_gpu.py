"""Tacotron (v1) on the GPU against the reference fixtures tests/golden/tacotron1_*.npz
(make_tacotron1_golden.py): stage parity, full batched parity, single rows, a 17-row batch across a
16-row boundary, set_r between calls and reloading weights. Weights are regenerated from the seeds."""
import json
import os

import numpy as np
import pytest
import torch

from tts_amd.spec import TacotronV1Config, tacotron_spec
from tts_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MEL_TOL = 1e-4
ALIGN_MARGIN = 1e-5
STOP_B = "decoder.stopnet.linear.bias"

_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


def _fixture(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return _cache[name]


def _state_dict(fx, r, seed=None):
    cfg = TacotronV1Config(**json.loads(str(fx["cfg"])))
    sd = synth_state_dict(tacotron_spec(cfg), int(fx[f"r{r}_seed"]) if seed is None else seed,
                          json.loads(str(fx["overrides"])))
    sd[STOP_B] = np.array([float(fx[f"r{r}_stop_bias"])], np.float32)
    return cfg, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _model(fx, r):
    """One loaded model per (fixture, seed), shared by the tests that do not reload it."""
    from tts_amd import Tacotron
    _dev()
    key = ("model", id(fx), int(fx[f"r{r}_seed"]))
    if key not in _cache:
        cfg, sd = _state_dict(fx, r)
        m = Tacotron(num_chars=cfg.num_chars, num_speakers=0, r=cfg.r, postnet_output_dim=cfg.postnet_output_dim,
                     attn_norm=cfg.attn_norm, memory_size=cfg.memory_size)
        m.load_state_dict(sd)
        _cache[key] = m.cuda().eval()
    m = _cache[key]
    m.decoder.set_r(r)
    m.decoder.max_decoder_steps = int(fx[f"r{r}_max_steps"])
    return m


def _n_utts(fx, r):
    return sum(1 for k in fx if k.startswith(f"r{r}_u") and k.endswith("_ids"))


def _batch(fx, r, rows):
    ids = [fx[f"r{r}_u{i}_ids"] for i in rows]
    batch = np.zeros((len(ids), max(len(x) for x in ids)), np.int64)
    for j, x in enumerate(ids):
        batch[j, :len(x)] = x
    return torch.from_numpy(batch).cuda(), [len(x) for x in ids]


def _infer(m, fx, r, rows, **kw):
    x, lens = _batch(fx, r, rows)
    dec, post, align, stop = m.inference(x, text_lengths=lens, **kw)
    return dec.cpu().numpy(), post.cpu().numpy(), align.cpu().numpy(), stop.cpu().numpy()


def _check(fx, r, rows, dec, post, align, stop, steps):
    """Row j of the outputs against fixture utterance rows[j] (the checks of _check_taco in
    test_gpu_parity.py)."""
    for j, i in enumerate(rows):
        k = f"r{r}_u{i}"
        S = len(fx[k + "_stop"])
        assert steps[j] == S, f"{k}: steps {steps[j]} != reference {S}"
        M = S * r
        ed, ep = np.abs(dec[j, :M] - fx[k + "_dec"]).max(), np.abs(post[j, :M] - fx[k + "_post"]).max()
        print(f"{k} row {j}: steps {S} dec err {ed:.2e} post err {ep:.2e}")
        assert ed <= MEL_TOL and ep <= MEL_TOL
        assert not post[j, M:].any() and not dec[j, M:].any()
        T = fx[k + "_align"].shape[1]
        a = align[j, :S, :T]
        assert np.abs(a - fx[k + "_align"]).max() <= 1e-5
        assert not align[j, S:].any() and not align[j, :, T:].any()
        sel = fx[k + "_top2"] > ALIGN_MARGIN
        assert np.array_equal(a.argmax(1)[sel], fx[k + "_align"].argmax(1)[sel])
        assert np.abs(stop[j, :S, 0] - fx[k + "_stop"]).max() <= 1e-4
        assert not stop[j, S:].any()


def test_stage_encoder():
    fx = _fixture("tacotron1_sigmoid")
    m = _model(fx, 5)
    x, lens = _batch(fx, 5, range(4))
    enc = m.encode(x, lens).cpu().numpy()
    ref = fx["r5_u1_enc"]
    err = np.abs(enc[1, :lens[1]] - ref).max()
    print(f"encoder err {err:.2e}")
    assert enc.shape == (4, 40, 256) and err <= MEL_TOL
    for j, n in enumerate(lens):
        assert not enc[j, n:].any() and enc[j, :n].any()
    alone = m.encode(x[1:2, :lens[1]]).cpu().numpy()
    assert np.array_equal(alone[0], enc[1, :lens[1]])


def test_stage_postnet():
    fx = _fixture("tacotron1_sigmoid")
    m = _model(fx, 5)
    decs = [fx[f"r5_u{i}_dec"] for i in range(4)]
    lens = [len(d) for d in decs]
    batch = np.zeros((4, max(lens), 80), np.float32)
    for j, d in enumerate(decs):
        batch[j, :len(d)] = d
    post = m.run_postnet(torch.from_numpy(batch).cuda(), lens).cpu().numpy()
    assert post.shape == (4, max(lens), 129)
    for j, n in enumerate(lens):
        err = np.abs(post[j, :n] - fx[f"r5_u{j}_post"]).max()
        print(f"postnet row {j} ({n} frames) err {err:.2e}")
        assert err <= MEL_TOL
        assert not post[j, n:].any()


@pytest.mark.parametrize("name, r", [("tacotron1_sigmoid", 5), ("tacotron1_sigmoid", 2), ("tacotron1_softmax_last", 5),
                                     ("tacotron1_mem3", 5), ("tacotron1_linear1025", 5)])
def test_full_parity_batched(name, r, capsys):
    fx = _fixture(name)
    m = _model(fx, r)
    rows = list(range(_n_utts(fx, r)))
    capsys.readouterr()
    dec, post, align, stop = _infer(m, fx, r, rows)
    printed = capsys.readouterr().out
    _check(fx, r, rows, dec, post, align, stop, m.last_steps)
    assert list(m.last_mel_lengths) == [s * r for s in m.last_steps]
    ms = int(fx[f"r{r}_max_steps"])
    at_max = [j for j in rows if len(fx[f"r{r}_u{j}_stop"]) == ms + 1]
    assert [j for j in rows if m.last_status[j] == 2] == at_max
    assert all(s in (1, 2) for s in m.last_status)
    assert printed.count("Decoder stopped with 'max_decoder_steps") == len(at_max)
    if (name, r) == ("tacotron1_sigmoid", 5):
        assert at_max == [3]  # the T = 40 utterance runs max_decoder_steps + 1 steps


@pytest.mark.parametrize("i", [0, 3])  # T = 1 and T = 40
def test_single_utterance_matches_and_is_batch_invariant(i):
    fx = _fixture("tacotron1_sigmoid")
    m = _model(fx, 5)
    full = _infer(m, fx, 5, range(4))
    steps_full = m.last_steps.copy()
    one = _infer(m, fx, 5, [i])
    _check(fx, 5, [i], *one, m.last_steps)
    S = int(m.last_steps[0])
    T = len(fx[f"r5_u{i}_ids"])
    assert steps_full[i] == S
    # every kernel computes a row from that row alone, in a fixed order: bit-identical
    assert np.array_equal(one[0][0, :S * 5], full[0][i, :S * 5])
    assert np.array_equal(one[1][0, :S * 5], full[1][i, :S * 5])
    assert np.array_equal(one[2][0, :S, :T], full[2][i, :S, :T])
    assert np.array_equal(one[3][0, :S], full[3][i, :S])


def test_seventeen_rows_cross_a_tile():
    fx = _fixture("tacotron1_sigmoid")
    m = _model(fx, 5)
    rows = [int(v) for v in np.random.RandomState(5).permutation(np.arange(17) % 3)]  # T = 1, 9, 23
    ms = np.full(17, int(fx["r5_max_steps"]))
    dec, post, align, stop = _infer(m, fx, 5, rows, max_decoder_steps=ms)
    _check(fx, 5, rows, dec, post, align, stop, m.last_steps)


def test_set_r_between_calls():
    fx = _fixture("tacotron1_sigmoid")
    assert int(fx["r5_seed"]) == int(fx["r2_seed"]) and float(fx["r5_stop_bias"]) == float(fx["r2_stop_bias"])
    m = _model(fx, 5)
    for r in (5, 2, 5):
        m.decoder.set_r(r)
        out = _infer(m, fx, r, range(4))
        _check(fx, r, range(4), *out, m.last_steps)
    m.decoder.set_r(6)
    with pytest.raises(ValueError, match="r=6"):
        m.inference(torch.zeros(1, 3, dtype=torch.long).cuda())
    m.decoder.set_r(5)


def test_reload_rebuilds_the_packed_copy():
    from tts_amd import Tacotron
    fx = _fixture("tacotron1_mem3")
    _dev()
    cfg, sd = _state_dict(fx, 5)
    _, other = _state_dict(fx, 5, seed=int(fx["r5_seed"]) + 1000)
    m = Tacotron(num_chars=cfg.num_chars, num_speakers=0, r=cfg.r, postnet_output_dim=cfg.postnet_output_dim,
                 attn_norm=cfg.attn_norm, memory_size=cfg.memory_size)
    m.load_state_dict(other)
    m = m.cuda().eval()
    m.decoder.max_decoder_steps = int(fx["r5_max_steps"])
    m.decoder.verbose = False
    before = _infer(m, fx, 5, [0, 1])
    m.load_state_dict(sd)
    after = _infer(m, fx, 5, [0, 1])
    _check(fx, 5, [0, 1], *after, m.last_steps)
    n = min(before[0].shape[1], after[0].shape[1])
    assert np.abs(before[0][:, :n] - after[0][:, :n]).max() > 100 * MEL_TOL


def test_inv_spectrogram_on_the_gpu_matches_the_cpu_path():
    """AudioProcessor(griffin_lim_device="gpu").inv_spectrogram against the CPU processor on the same
    phase numbers: same length, and the spectral convergence of the GPU waveform (measured with the
    CPU float64 STFT) within 1e-3 relative of the CPU waveform's, the bound
    tests/test_griffin_lim.py holds the same Griffin-Lim kernels to on the mel path."""
    from tts_amd.audio import AudioProcessor
    _dev()
    audio = dict(fft_size=1024, win_length=1024, hop_length=256, sample_rate=22050, preemphasis=0.0, ref_level_db=20,
                 power=1.5, griffin_lim_iters=30, num_mels=80, mel_fmin=50.0, mel_fmax=7600.0, spec_gain=20,
                 signal_norm=True, min_level_db=-100, symmetric_norm=True, max_norm=4.0, clip_norm=True)
    cpu, gpu = AudioProcessor(**audio), AudioProcessor(**dict(audio, griffin_lim_device="gpu"))
    t = np.arange(256 * 24) / 22050.0
    wav = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * (500.0 + 900.0 * t) * t)
    spec = cpu.spectrogram(wav)
    u = np.random.RandomState(3).rand(*spec.shape)

    class Rng:
        def rand(self, *shape):
            assert tuple(shape) == u.shape
            return u

    ref = cpu.inv_spectrogram(spec, Rng())
    y = gpu.inv_spectrogram(spec, Rng())
    assert isinstance(y, np.ndarray) and y.shape == ref.shape and np.isfinite(y).all()
    S = cpu._db_to_amp(cpu._denormalize(spec)) ** cpu.power  # the magnitudes Griffin-Lim is given

    def conv(w):
        return np.linalg.norm(np.abs(cpu._stft(w)) - S) / np.linalg.norm(S)

    sc_gpu, sc_cpu = conv(y.astype(np.float64)), conv(ref)
    print(f"spectral convergence: gpu {sc_gpu:.6e} cpu {sc_cpu:.6e}")
    assert abs(sc_gpu - sc_cpu) <= 1e-3 * sc_cpu
