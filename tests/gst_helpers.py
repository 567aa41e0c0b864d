"""Fixture plumbing of the Global Style Token tests (tests/golden/make_gst_golden.py): the model of a
``taco_gst_*`` fixture, regenerated from its seed and gains."""
import json

import numpy as np
import torch

from helpers import load_fixture
from tts_amd.spec import TacotronConfig, tacotron2_spec
from tts_amd.weights import synth_state_dict


def gst_fixture(tag):
    fx = load_fixture("taco_gst_" + tag)
    return fx, TacotronConfig(**json.loads(str(fx["cfg"])))


def gst_state_dict(fx, cfg):
    sd = synth_state_dict(tacotron2_spec(cfg), int(fx["seed"]), json.loads(str(fx["overrides"])))
    sd["decoder.stopnet.1.linear_layer.bias"] = np.array([float(fx["stop_bias"])], np.float32)
    return sd


def build_gst_taco(cfg, sd=None, device="cpu"):
    from tts_amd import Tacotron2
    m = Tacotron2(num_chars=cfg.num_chars, num_speakers=cfg.num_speakers, r=cfg.r, attn_norm=cfg.attn_norm,
                  double_decoder_consistency=cfg.double_decoder_consistency, ddc_r=cfg.ddc_r,
                  speaker_embedding_dim=cfg.speaker_embedding_dim, prenet_type=cfg.prenet_type, gst=cfg.gst,
                  gst_embedding_dim=cfg.gst_embedding_dim, gst_num_heads=cfg.gst_num_heads,
                  gst_style_tokens=cfg.gst_style_tokens, gst_use_speaker_embedding=cfg.gst_use_speaker_embedding)
    if sd is not None:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(device).eval()
