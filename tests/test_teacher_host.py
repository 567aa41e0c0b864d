"""Host-side checks of the teacher-forced ``Tacotron2.forward`` (no GPU): what it raises, in which
order, and that the library exports its entry point."""
import ctypes
import os
import re

import pytest
import torch

from tts_amd import Tacotron, Tacotron2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(B=2, T=6, M=8):
    return torch.ones(B, T, dtype=torch.long), torch.full((B,), T), torch.zeros(B, M, 80)


def _model(**kw):
    return Tacotron2(num_chars=129, r=7, attn_norm="sigmoid", **kw).eval()


def test_eval_forward_on_a_cpu_model_has_no_fallback():
    m = _model()
    m.decoder.set_r(2)
    text, lens, mel = _args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward(text, lens, mel)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(text, lens, mel, torch.tensor([8, 3]))


def test_training_forward_stays_out_of_scope():
    m = _model().train()
    with pytest.raises(NotImplementedError, match="training forward"):
        m.forward(*_args())
    with pytest.raises(NotImplementedError, match="training forward"):
        Tacotron(num_chars=30, num_speakers=0).eval()(torch.zeros(1, 4, dtype=torch.long))  # v1 is untouched


def test_argument_errors_come_before_the_device_check():
    m = _model()
    m.decoder.set_r(2)
    text, lens, mel = _args()
    with pytest.raises(RuntimeError, match="multiple of r"):  # the reference's view() fails here too
        m.forward(text, lens, torch.zeros(2, 7, 80))
    with pytest.raises(ValueError, match="mel_specs"):  # channel count
        m.forward(text, lens, torch.zeros(2, 8, 79))
    with pytest.raises(ValueError, match="mel_specs"):  # forward is teacher-forced
        m.forward(text, lens)
    with pytest.raises(ValueError, match="one row per row"):
        m.forward(text, lens, torch.zeros(3, 8, 80))
    with pytest.raises(ValueError, match="text_lengths"):
        m.forward(text, torch.tensor([6]), mel)
    for bad in ([0, 8], [8, 9], [8]):
        with pytest.raises(ValueError, match="mel_lengths"):
            m.forward(text, lens, mel, torch.tensor(bad))


def test_speaker_arguments_are_checked():
    m = _model(num_speakers=4)
    m.decoder.set_r(2)
    text, lens, mel = _args()
    with pytest.raises(ValueError, match="speaker_ids"):
        m.forward(text, lens, mel)
    with pytest.raises(IndexError):
        m.forward(text, lens, mel, speaker_ids=torch.tensor([0, 4]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward(text, lens, mel, speaker_ids=torch.tensor([0, 3]))


@pytest.mark.parametrize("kw,name", [({"attn_win": True}, "attn_win"), ({"forward_attn": True}, "forward_attn"),
                                     ({"attn_type": "graves"}, "graves")])
def test_out_of_scope_attention_options_are_named(kw, name):
    m = _model(**kw)  # the constructor accepts them: inference() supports them
    with pytest.raises(NotImplementedError, match=name):
        m.forward(*_args())


def test_entry_point_declared_typed_and_exported():
    from tts_amd._lib import LIB_PATH, SIGNATURES
    header = open(os.path.join(ROOT, "include", "ttship.h")).read()
    assert re.search(r"\bint tts_taco_forward\(tts_ctx\* ctx", header)
    assert "tts_taco_forward" in {n for n, _, _ in SIGNATURES}
    assert hasattr(ctypes.CDLL(LIB_PATH), "tts_taco_forward")
