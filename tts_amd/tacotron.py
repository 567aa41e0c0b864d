"""Drop-in ``Tacotron`` (v1) whose ``inference`` runs on MI355X through ``libttship.so``.

Mirrors the reference surface: the constructor signature of ``TTS/tts/models/tacotron.py:10-39``,
checkpoint keys (``load_state_dict(cp['model'])``), ``.cuda()`` / ``.eval()``,
``decoder.set_r(r)``, ``decoder.max_decoder_steps`` (500, ``layers/tacotron.py:299``) and
``inference(characters, speaker_ids, style_mel, speaker_embeddings)`` returning
``(decoder_outputs (B, M, 80), postnet_outputs (B, M, postnet_output_dim), alignments (B, S, T),
stop_tokens (B, S, 1))`` (``models/tacotron.py:150-172``).

In scope: the single-speaker model with original (location-sensitive) attention, sigmoid or
softmax normalisation, the original prenet, any ``memory_size`` and any ``r`` in ``[1, r_init]``.
Everything else raises ``NotImplementedError`` naming the argument.

Batching (this project's own, as for ``Tacotron2``): ``characters`` may hold B > 1 padded rows with
``text_lengths``; row i of the outputs equals the reference B = 1 call on utterance i. The
per-utterance lengths are in ``last_steps`` / ``last_mel_lengths`` after the call, ``last_status``
is 1 (stop rule) or 2 (``max_decoder_steps`` reached); padded positions are zero.
"""

from typing import Optional, Sequence

import numpy as np
import torch

from .params import Container, host_tensors, populate
from .spec import TacotronV1Config, tacotron_spec
from .tacotron_host import TacotronHost

BATCH_LIMIT = 64  # rows per library call (ttship.h)


class Decoder(Container):
    """Holds the decoder parameters plus the runtime knobs the reference exposes."""

    def __init__(self, r: int, memory_size: int, frame_channels: int = 80):
        super().__init__()
        self.r_init = r
        self.r = r
        self.frame_channels = frame_channels
        self.max_decoder_steps = 500
        self.use_memory_queue = memory_size > 0
        self.memory_size = memory_size if memory_size > 0 else r
        self.query_dim = 256

    def set_r(self, new_r):
        self.r = int(new_r)


class Tacotron(TacotronHost):
    _slot = "tacotron1"

    def __init__(self, num_chars, num_speakers, r=5, postnet_output_dim=1025, decoder_output_dim=80,
                 attn_type="original", attn_win=False, attn_norm="sigmoid", prenet_type="original",
                 prenet_dropout=True, forward_attn=False, trans_agent=False, forward_attn_mask=False,
                 location_attn=True, attn_K=5, separate_stopnet=True, bidirectional_decoder=False,
                 double_decoder_consistency=False, ddc_r=None, encoder_in_features=256,
                 decoder_in_features=256, speaker_embedding_dim=None, gst=False, gst_embedding_dim=256,
                 gst_num_heads=4, gst_style_tokens=10, memory_size=5, gst_use_speaker_embedding=False):
        super().__init__()
        unsupported = []
        if gst:
            unsupported.append("gst=True")
        if num_speakers > 1:
            unsupported.append(f"num_speakers={num_speakers}")
        if attn_type != "original":
            unsupported.append(f"attn_type={attn_type}")
        if attn_win:
            unsupported.append("attn_win")
        if forward_attn:
            unsupported.append("forward_attn")
        if trans_agent:
            unsupported.append("trans_agent")
        if prenet_type != "original":
            unsupported.append(f"prenet_type={prenet_type}")
        if not location_attn:
            unsupported.append("location_attn=False")
        if encoder_in_features != 256 or decoder_in_features != 256:
            unsupported.append("non-default encoder_in_features/decoder_in_features")
        if decoder_output_dim != 80:
            unsupported.append(f"decoder_output_dim={decoder_output_dim}")
        if attn_norm not in ("sigmoid", "softmax"):
            raise ValueError("Unknown value for attention norm type")
        if unsupported:
            raise NotImplementedError("tts_amd Tacotron does not implement: " + ", ".join(unsupported) +
                                      " (SURVEY.md §8f)")
        self.num_chars = num_chars
        self.num_speakers = num_speakers
        self.r = r
        self.attn_norm = attn_norm
        self.postnet_output_dim = int(postnet_output_dim)
        self.decoder_output_dim = decoder_output_dim
        self.bidirectional_decoder = bool(bidirectional_decoder)
        self.double_decoder_consistency = bool(double_decoder_consistency)
        self.gst = False
        self.cfg = TacotronV1Config(num_chars=num_chars, r=r, postnet_output_dim=self.postnet_output_dim,
                                    memory_size=int(memory_size), attn_norm=attn_norm,
                                    double_decoder_consistency=self.double_decoder_consistency,
                                    ddc_r=ddc_r if ddc_r is not None else r,
                                    bidirectional_decoder=self.bidirectional_decoder)
        self.decoder = Decoder(r, int(memory_size), decoder_output_dim)
        spec = tacotron_spec(self.cfg)
        populate(self, spec)
        # state_dict order = the reference's registration order (the decoder holder was made first)
        order = list(dict.fromkeys(name.split(".")[0] for name, _, _ in spec))
        for k in order:
            self._modules[k] = self._modules.pop(k)

    def _load(self, eng):
        eng.load_tacotron1(host_tensors(self, skip_prefixes=("coarse_decoder.", "decoder_backward.")),
                           self.num_chars, self.decoder.r_init, self.cfg.memory_size, self.attn_norm,
                           self.postnet_output_dim)

    def _text_args(self, characters, text_lengths, max_decoder_steps):
        args = super()._text_args(characters, text_lengths, max_decoder_steps)
        if args[4].min() < 1:
            raise ValueError("max_decoder_steps must be >= 1")
        return args

    @torch.no_grad()
    def inference(self, characters, speaker_ids=None, style_mel=None, speaker_embeddings=None,
                  text_lengths: Optional[Sequence[int]] = None, max_decoder_steps=None):
        """speaker_ids / style_mel / speaker_embeddings are ignored, as the reference ignores them
        for a single-speaker model without GST (models/tacotron.py:154-166)."""
        dev, eng, text, lens, ms, r = self._text_args(characters, text_lengths, max_decoder_steps)
        B = text.shape[0]
        outs = []
        with eng.lock:
            self._sync(eng)
            for b0 in range(0, B, BATCH_LIMIT):
                b1 = min(B, b0 + BATCH_LIMIT)
                Tn = int(lens[b0:b1].max())
                sub = text[b0:b1, :Tn].contiguous()
                S_cap = int(ms[b0:b1].max()) + 1  # a row that never stops takes max_decoder_steps + 1 steps
                dec, post, align, stop = self._out_tensors(b1 - b0, S_cap, r, Tn, dev)
                steps, status = eng.tacotron1_infer(sub, lens[b0:b1], r, ms[b0:b1], S_cap, dec, post, align, stop)
                outs.append((dec, post, align, stop, steps, status))
        return self._assemble(outs, text.shape, r, dev)

    # stage entry points (parity by stage)
    @torch.no_grad()
    def encode(self, characters, text_lengths=None):
        """Encoder outputs (B, T, 256) = Encoder(embedding(characters)), zero past each row's length."""
        dev, eng, text, lens, _, _ = self._text_args(characters, text_lengths, None)
        out = torch.empty(text.shape[0], text.shape[1], 256, device=dev, dtype=torch.float32)
        with eng.lock:
            self._sync(eng)
            eng.tacotron1_encoder(text, lens, out)
        return out

    @torch.no_grad()
    def run_postnet(self, decoder_outputs, mel_lengths=None):
        """last_linear(PostCBHG(decoder_outputs)) on (B, M, 80) frames -> (B, M, postnet_output_dim)."""
        dev = self.device
        eng = self._engine()
        dec = torch.as_tensor(decoder_outputs).to(dev, torch.float32).contiguous()
        B, M, _ = dec.shape
        lens = np.full(B, M, np.int64) if mel_lengths is None else np.asarray(mel_lengths, dtype=np.int64)
        out = torch.empty(B, M, self.postnet_output_dim, device=dev, dtype=torch.float32)
        with eng.lock:
            self._sync(eng)
            eng.tacotron1_postnet(dec, lens, out)
        return out
