"""Host-side tests of Global Style Tokens on multi-speaker Tacotron2 (no GPU): the constructor fence,
the checkpoint keys, argument checks that come before the device check, the C ABI names, the CLI's
``--gst_style`` parsing, and a float64 numpy restatement of the GST module (gst_layers.py) that
reproduces the fixtures' style embeddings within their recorded fp32-vs-fp64 drift."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from gst_helpers import build_gst_taco, gst_fixture, gst_state_dict
from helpers import GOLDEN
from tts_amd import Tacotron2
from tts_amd.spec import TacotronConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["tts_taco_gst_info", "tts_taco_style_mel", "tts_taco_style_tokens", "tts_taco_infer_style",
               "tts_taco_forward_style"]


def test_gst_is_accepted_for_multi_speaker_models_only():
    m = Tacotron2(num_chars=129, num_speakers=4, r=2, gst=True)
    assert tuple(m.state_dict()["decoder.attention.inputs_layer.linear_layer.weight"].shape) == (128, 1536)
    assert tuple(m.state_dict()["gst_layer.style_token_layer.attention.W_query.weight"].shape) == (512, 256)
    m = Tacotron2(num_chars=129, num_speakers=4, r=2, gst=True, speaker_embedding_dim=256,
                  gst_use_speaker_embedding=True)
    assert tuple(m.state_dict()["gst_layer.style_token_layer.attention.W_query.weight"].shape) == (512, 512)
    for n in (0, 1):
        with pytest.raises(NotImplementedError, match="single-speaker"):
            Tacotron2(num_chars=129, num_speakers=n, gst=True)


@pytest.mark.parametrize("kw,name", [(dict(gst_embedding_dim=384), "gst_embedding_dim"),
                                     (dict(gst_num_heads=3), "gst_num_heads"),
                                     (dict(gst_style_tokens=33), "gst_style_tokens"),
                                     (dict(gst_style_tokens=0), "gst_style_tokens")])
def test_unsupported_gst_shapes_are_named(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        Tacotron2(num_chars=129, num_speakers=4, gst=True, **kw)


@pytest.mark.parametrize("G,heads,tokens", [(128, 2, 1), (256, 8, 32), (512, 4, 10)])
def test_supported_gst_shapes_build(G, heads, tokens):
    m = Tacotron2(num_chars=129, num_speakers=2, gst=True, gst_embedding_dim=G, gst_num_heads=heads,
                  gst_style_tokens=tokens)
    assert tuple(m.state_dict()["gst_layer.style_token_layer.style_tokens"].shape) == (tokens, G // heads)


@pytest.mark.parametrize("tag", ["ext", "tab"])
def test_state_dict_keys_and_shapes_equal_the_references(tag):
    _, cfg = gst_fixture(tag)
    ref = json.load(open(os.path.join(GOLDEN, "taco_gst_keys.json")))[tag]
    mine = [(k, list(v.shape)) for k, v in build_gst_taco(cfg).state_dict().items()]
    assert dict(mine) == {k: s for k, s in ref}
    # the gst_layer block in the reference's own order
    assert [k for k, _ in mine if k.startswith("gst_layer.")] == [k for k, _ in ref if k.startswith("gst_layer.")]


def test_old_configs_without_gst_fields_still_load():
    cfg = TacotronConfig(**{"num_chars": 129, "r": 2, "num_speakers": 4})
    assert not cfg.gst and cfg.gst_dim == 0 and cfg.decoder_in == 1024


def _cpu_model(**kw):
    return Tacotron2(num_chars=129, num_speakers=4, r=2, gst=True, gst_style_tokens=10, **kw).eval()


def test_style_argument_errors_come_before_the_device_check():
    m = _cpu_model()
    text, spk = torch.ones(2, 5, dtype=torch.long), torch.tensor([0, 1])
    with pytest.raises(ValueError, match="one row per utterance"):
        m.inference(text, speaker_ids=spk, style_mel=torch.zeros(3, 7, 80))
    with pytest.raises(ValueError, match="style_lengths"):
        m.inference(text, speaker_ids=spk, style_mel=torch.zeros(2, 7, 80), style_lengths=[7, 8])
    with pytest.raises(ValueError, match="style_lengths"):
        m.inference(text, speaker_ids=spk, style_mel=torch.zeros(2, 7, 80), style_lengths=[0, 7])
    with pytest.raises(ValueError, match="style_lengths"):
        m.inference(text, speaker_ids=spk, style_mel=torch.zeros(2, 7, 80), style_lengths=[7])
    with pytest.raises(ValueError, match="style_mel"):
        m.inference(text, speaker_ids=spk, style_mel=torch.zeros(2, 7, 79))
    for bad in ({"10": 0.1}, {"0": 0.2, "-11": 0.1}):
        with pytest.raises(IndexError):
            m.inference(text, speaker_ids=spk, style_mel=bad)
    with pytest.raises(IndexError):
        m.style_embedding({"10": 1.0})


@pytest.mark.parametrize("style", [None, {"0": 0.3, "-1": 0.1}, torch.zeros(1, 7, 80), torch.zeros(2, 80, 7)])
def test_no_cpu_fallback(style):
    m = _cpu_model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(torch.ones(2, 5, dtype=torch.long), speaker_ids=torch.tensor([0, 1]), style_mel=style)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.style_embedding(style)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward(torch.ones(2, 5, dtype=torch.long), [5, 5], torch.zeros(2, 4, 80), speaker_ids=torch.tensor([0, 1]))


def test_a_model_without_gst_still_refuses_a_style():
    m = Tacotron2(num_chars=129, num_speakers=4, r=2)
    with pytest.raises(NotImplementedError, match="gst=True"):
        m.inference(torch.ones(1, 5, dtype=torch.long), speaker_ids=torch.tensor([0]), style_mel=torch.zeros(1, 7, 80))
    with pytest.raises(NotImplementedError, match="gst=True"):
        m.style_embedding(torch.zeros(1, 7, 80))


def test_query_speaker_embeddings_are_required_when_the_query_takes_them():
    m = _cpu_model(speaker_embedding_dim=256, gst_use_speaker_embedding=True)
    with pytest.raises(ValueError, match="speaker_embeddings"):
        m.style_embedding(torch.zeros(1, 7, 80))
    with pytest.raises(ValueError, match="one row per style mel"):
        m.style_embedding(torch.zeros(1, 7, 80), speaker_embeddings=torch.zeros(2, 256))


def test_new_entries_declared_typed_and_exported():
    from tts_amd._lib import LIB_PATH, SIGNATURES
    header = open(os.path.join(ROOT, "include", "ttship.h")).read()
    typed = {n for n, _, _ in SIGNATURES}
    lib = ctypes.CDLL(LIB_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\(tts_ctx\* ctx" % name, header), name
        assert name in typed, name
        assert hasattr(lib, name), name


def test_cli_gst_style_parsing():
    from tts_amd.synthesize import parse_gst_style
    C = {"gst": {"gst_style_tokens": 10, "gst_style_input": "ref.wav"}}
    assert parse_gst_style(None, C) == "ref.wav"
    assert parse_gst_style('{"0": 0.3, "9": -0.1}', C) == {"0": 0.3, "9": -0.1}
    assert parse_gst_style("some/style.wav", C) == "some/style.wav"
    with pytest.raises(RuntimeError, match="number of GST"):
        parse_gst_style('{"10": 0.3}', C)


def test_synthesis_hands_the_style_to_the_model():
    """A dict passes through; a wav path becomes the (1, num_mels, N) melspectrogram (untransposed)."""
    from tts_amd.synthesis import synthesis
    seen = {}

    class Model:
        def inference(self, inputs, style_mel=None, speaker_ids=None, speaker_embeddings=None):
            seen["style"] = style_mel
            z = torch.zeros(1, 2, 80)
            return z, z, torch.zeros(1, 1, inputs.shape[1]), torch.zeros(1, 1, 1)

    class Ap:
        sample_rate = 22050

        def load_wav(self, path, sr=None):
            return np.zeros(4, np.float32)

        def melspectrogram(self, wav):
            return np.arange(80 * 3, dtype=np.float32).reshape(80, 3)

    C = {"model": "Tacotron2", "use_gst": True, "text_cleaner": "basic_cleaners", "use_phonemes": False,
         "enable_eos_bos_chars": False}
    synthesis(Model(), "ab", C, False, Ap(), speaker_id=0, style_wav={"1": 0.2})
    assert seen["style"] == {"1": 0.2}
    synthesis(Model(), "ab", C, False, Ap(), speaker_id=0, style_wav="x.wav")
    assert tuple(seen["style"].shape) == (1, 80, 3)
    synthesis(Model(), "ab", C, False, Ap(), speaker_id=0)
    assert seen["style"] is None


# ---- the GST module in float64 numpy (gst_layers.py:27-176) ----

def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gst_numpy(sd, G, heads, mel, spk=None):
    p = "gst_layer."
    w = {k[len(p):]: np.asarray(v, np.float64) for k, v in sd.items() if k.startswith(p)}
    x = mel.reshape(1, -1, 80).astype(np.float64)  # (C = 1, frames, 80)
    for l in range(6):
        W, b = w[f"encoder.convs.{l}.weight"], w[f"encoder.convs.{l}.bias"]
        _, H, Wd = x.shape
        Ho, Wo = (H + 1) // 2, (Wd + 1) // 2
        xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
        y = np.zeros((W.shape[0], Ho, Wo))
        for kh in range(3):
            for kw in range(3):
                y += np.einsum("oc,chw->ohw", W[:, :, kh, kw], xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2])
        y += b[:, None, None]
        bn = f"encoder.bns.{l}."
        y = (y - w[bn + "running_mean"][:, None, None]) / np.sqrt(w[bn + "running_var"][:, None, None] + 1e-5)
        x = np.maximum(y * w[bn + "weight"][:, None, None] + w[bn + "bias"][:, None, None], 0.0)
    seq = x.transpose(1, 0, 2).reshape(x.shape[1], -1)  # (steps, 128 channels x 2 bins)
    Hg = G // 2
    r = "encoder.recurrence."
    h = np.zeros(Hg)
    for xt in seq:
        gi = w[r + "weight_ih_l0"] @ xt + w[r + "bias_ih_l0"]
        gh = w[r + "weight_hh_l0"] @ h + w[r + "bias_hh_l0"]
        rg, z = _sigmoid(gi[:Hg] + gh[:Hg]), _sigmoid(gi[Hg:2 * Hg] + gh[Hg:2 * Hg])
        n = np.tanh(gi[2 * Hg:] + rg * gh[2 * Hg:])
        h = (1 - z) * n + z * h
    a = "style_token_layer.attention."
    qin = h if spk is None else np.concatenate([h, np.asarray(spk, np.float64)])
    tok = np.tanh(w["style_token_layer.style_tokens"])
    q, k, v = w[a + "W_query.weight"] @ qin, tok @ w[a + "W_key.weight"].T, tok @ w[a + "W_value.weight"].T
    dk = G // heads
    out = np.zeros(G)
    for hd in range(heads):
        s = k[:, hd * dk:(hd + 1) * dk] @ q[hd * dk:(hd + 1) * dk] / dk ** 0.5
        e = np.exp(s - s.max())
        out[hd * dk:(hd + 1) * dk] = (e / e.sum()) @ v[:, hd * dk:(hd + 1) * dk]
    return out, v


@pytest.mark.parametrize("tag", ["ext", "tab"])
def test_numpy_restatement_reproduces_the_fixture_within_its_drift(tag):
    fx, cfg = gst_fixture(tag)
    sd = gst_state_dict(fx, cfg)
    drift = fx["style_drift64"]
    for i, N in enumerate(fx["style_n"]):
        spk = fx["style_spk"][i] if cfg.gst_query_speaker_dim else None
        out, v = gst_numpy(sd, cfg.gst_embedding_dim, cfg.gst_num_heads, fx[f"style_mel_{N}"], spk)
        err = np.abs(out - fx[f"style_{N}"]).max()
        assert err <= drift[i] * 1.001 + 1e-12, (N, err, drift[i])
    d = np.zeros(cfg.gst_embedding_dim)
    for k, a in json.loads(str(fx["style_dict"])).items():
        d = d + v[int(k)] * a
    assert np.abs(d - fx["dict_style"]).max() <= drift[-1] * 1.001 + 1e-12
    assert float(fx["style_tol"]) == pytest.approx(8 * drift.max())
