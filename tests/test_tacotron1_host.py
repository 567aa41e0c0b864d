"""Host-side checks of the Tacotron (v1) surface: state_dict layout, the constructor's fences, the
factory, the linear-spectrogram audio path and the exported C symbols. No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tts_amd import Tacotron, setup_model
from tts_amd.audio import AudioProcessor
from tts_amd.factories import AttrDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("memory_size", [5, -1])
def test_state_dict_matches_reference_keys(memory_size):
    ref = json.load(open(os.path.join(GOLDEN, "tacotron1_keys.json")))[f"memory_size_{memory_size}"]
    m = Tacotron(num_chars=129, num_speakers=0, r=5, postnet_output_dim=1025, memory_size=memory_size)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(ref) == 252
    assert got == ref


def test_ddc_and_bidirectional_checkpoints_are_accepted():
    m = Tacotron(num_chars=50, num_speakers=0, r=5, double_decoder_consistency=True, ddc_r=7,
                 bidirectional_decoder=True)
    sd = m.state_dict()
    assert sd["coarse_decoder.proj_to_mel.weight"].shape == (560, 256)
    assert sd["decoder_backward.proj_to_mel.weight"].shape == (400, 256)
    m.load_state_dict(sd)


@pytest.mark.parametrize("kw, named", [
    (dict(gst=True), "gst"),
    (dict(num_speakers=4), "num_speakers"),
    (dict(attn_type="graves"), "attn_type"),
    (dict(attn_win=True), "attn_win"),
    (dict(forward_attn=True), "forward_attn"),
    (dict(trans_agent=True), "trans_agent"),
    (dict(prenet_type="bn"), "prenet_type"),
    (dict(location_attn=False), "location_attn"),
])
def test_out_of_scope_arguments_raise(kw, named):
    args = dict(num_chars=129, num_speakers=0)
    args.update(kw)
    with pytest.raises(NotImplementedError, match=named):
        Tacotron(**args)


def _config(**over):
    c = AttrDict(model="Tacotron", r=5, memory_size=5, use_gst=False,
                 gst=dict(gst_embedding_dim=256, gst_num_heads=4, gst_style_tokens=10,
                          gst_use_speaker_embedding=False),
                 attention_type="original", windowing=False, attention_norm="sigmoid", prenet_type="original",
                 prenet_dropout=True, use_forward_attn=False, transition_agent=False, forward_attn_mask=False,
                 location_attn=True, attention_heads=5, separate_stopnet=True, bidirectional_decoder=False,
                 double_decoder_consistency=False, ddc_r=None,
                 audio=dict(fft_size=1024, num_mels=80, sample_rate=22050))
    c.update(over)
    return c


def test_setup_model_builds_tacotron(capsys):
    m = setup_model(61, 0, _config())
    assert isinstance(m, Tacotron)
    assert m.postnet_output_dim == 513
    assert m.last_linear.weight.shape == (513, 256)
    assert m.decoder.r == 5 and m.decoder.r_init == 5 and m.decoder.max_decoder_steps == 500
    assert m.decoder.prenet.linear_layers._modules["0"].linear_layer.weight.shape == (256, 400)
    m2 = setup_model(61, 0, _config(memory_size=-1, r=3))
    assert m2.decoder.prenet.linear_layers._modules["0"].linear_layer.weight.shape == (256, 80)
    assert m2.decoder.proj_to_mel.weight.shape == (240, 256)
    m2.decoder.set_r(2)
    assert m2.decoder.r == 2 and m2.decoder.r_init == 3


def test_cpu_model_has_no_fallback_and_forward_raises():
    m = Tacotron(num_chars=30, num_speakers=0).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="training forward"):
        m(torch.zeros(1, 4, dtype=torch.long))


def _ap(**kw):
    args = dict(sample_rate=22050, num_mels=80, min_level_db=-100, frame_shift_ms=None, frame_length_ms=None,
                hop_length=256, win_length=1024, ref_level_db=20, fft_size=1024, power=1.5, preemphasis=0.0,
                signal_norm=True, symmetric_norm=True, max_norm=4.0, mel_fmin=0.0, mel_fmax=8000.0, spec_gain=20,
                stft_pad_mode="reflect", clip_norm=True, griffin_lim_iters=4, do_trim_silence=False, verbose=False)
    args.update(kw)
    return AudioProcessor(**args)


@pytest.mark.parametrize("preemphasis", [0.0, 0.97])
def test_inv_spectrogram_round_trip(preemphasis):
    ap = _ap(preemphasis=preemphasis)
    t = np.arange(256 * 20) / 22050.0
    wav = 0.4 * np.sin(2 * np.pi * 440.0 * t)
    S = ap.spectrogram(wav)
    assert S.shape == (513, 21)
    out = ap.inv_spectrogram(S, rng=np.random.RandomState(0))
    assert out.shape == (256 * 20,)
    assert np.isfinite(out).all() and np.abs(out).max() > 1e-3


def test_synthesis_inv_spectrogram_picks_the_linear_branch():
    from tts_amd import synthesis

    class Ap:
        def inv_spectrogram(self, S):
            return ("linear", S.shape)

        def inv_melspectrogram(self, S):
            return ("mel", S.shape)

    post = np.zeros((7, 513), np.float32)
    assert synthesis.inv_spectrogram(post, Ap(), {"model": "Tacotron"}) == ("linear", (513, 7))
    assert synthesis.inv_spectrogram(post[:, :80], Ap(), {"model": "Tacotron2"}) == ("mel", (80, 7))


def test_run_model_torch_accepts_the_model():
    from tts_amd import synthesis

    class M:
        def inference(self, inputs, speaker_ids=None, speaker_embeddings=None):
            return ("dec", "post", "align", "stop")

    assert synthesis.run_model_torch(M(), None, {"model": "Tacotron"}, False) == ("dec", "post", "align", "stop")


def test_c_symbols_exported_and_declared():
    from tts_amd._lib import LIB_PATH, SIGNATURES
    names = ["tts_tacotron1_set_tensor", "tts_tacotron1_finalize", "tts_tacotron1_infer", "tts_tacotron1_encoder",
             "tts_tacotron1_postnet"]
    header = open(os.path.join(ROOT, "include", "ttship.h")).read()
    typed = {n for n, _, _ in SIGNATURES}
    lib = ctypes.CDLL(LIB_PATH)
    for n in names:
        assert re.search(r"\bint %s\(tts_ctx\* ctx" % n, header), n
        assert n in typed
        assert hasattr(lib, n)
