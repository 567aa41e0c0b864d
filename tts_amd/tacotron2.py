"""Drop-in ``Tacotron2`` whose ``inference`` runs on MI355X through ``libttship.so``.

Mirrors the reference surface used by ``TTS/server/synthesizer.py:43-79`` and
``TTS/tts/utils/synthesis.py:48-67``: the constructor signature of
``TTS/tts/models/tacotron2.py:10-37``, checkpoint keys (``load_state_dict(cp['model'])``),
``.cuda()`` / ``.eval()``, ``decoder.set_r(r)`` (``layers/tacotron2.py:208-209``),
``decoder.max_decoder_steps`` (``:156``) and ``inference(text, speaker_ids, style_mel,
speaker_embeddings)`` returning ``(decoder_outputs (B,M,80), postnet_outputs (B,M,80),
alignments (B,S,T), stop_tokens (B,S,1))`` (``models/tacotron2.py:142-163``).

Batching (new, optional): ``text`` may hold B > 1 padded rows with ``text_lengths``; row i
of the outputs equals the reference B=1 call on utterance i (the reference itself cannot
run B > 1: ``layers/tacotron2.py:362``). Per-utterance lengths are in ``last_steps`` /
``last_mel_lengths`` after the call; padded positions are zero.
"""

from typing import Optional, Sequence

import numpy as np
import torch

from .params import Container, host_tensors, populate, row_lengths
from .spec import TacotronConfig, tacotron2_spec
from .tacotron_host import TacotronHost

BATCH_LIMIT = 64
SPEAKER_BATCH_LIMIT = 64  # multi-speaker / decoder variants run on the persistent decoder (<= 64 rows)


class Decoder(Container):
    """Holds decoder parameters plus the runtime knobs the reference exposes."""

    def __init__(self, r: int, frame_channels: int = 80):
        super().__init__()
        self.r_init = r
        self.r = r
        self.frame_channels = frame_channels
        self.max_decoder_steps = 1000
        self.stop_threshold = 0.5

    def set_r(self, new_r):
        self.r = int(new_r)


class VocodedResult:
    """A submitted ``Tacotron2.inference_vocoded_submit`` call. ``outputs`` holds the decode's
    (decoder_outputs, postnet_outputs, alignments, stop_tokens), ready on return; the waveforms are
    final once ``result()`` has returned (it completes the library ticket)."""

    def __init__(self, outputs, wav, eng=None, ticket=None):
        self.outputs = outputs
        self._wav = wav
        self._eng, self._ticket = eng, ticket

    def result(self):
        if self._ticket is not None:
            with self._eng.lock:
                self._eng.taco_mbmelgan_finish(self._ticket, self._wav.device)
            self._ticket = None
        return tuple(self.outputs) + (self._wav,)


class Tacotron2(TacotronHost):
    _slot = "taco"

    def __init__(self, num_chars, num_speakers=0, r=7, postnet_output_dim=80, decoder_output_dim=80,
                 attn_type="original", attn_win=False, attn_norm="softmax", prenet_type="original",
                 prenet_dropout=True, forward_attn=False, trans_agent=False, forward_attn_mask=False,
                 location_attn=True, attn_K=5, separate_stopnet=True, bidirectional_decoder=False,
                 double_decoder_consistency=False, ddc_r=None, encoder_in_features=512,
                 decoder_in_features=512, speaker_embedding_dim=None, gst=False, gst_embedding_dim=512,
                 gst_num_heads=4, gst_style_tokens=10, gst_use_speaker_embedding=False):
        super().__init__()
        unsupported = []
        if gst and num_speakers <= 1:
            unsupported.append("GST on a single-speaker model (gst=True needs num_speakers > 1)")
        elif gst:
            if gst_embedding_dim not in (128, 256, 512):
                unsupported.append(f"gst_embedding_dim={gst_embedding_dim} (128, 256 or 512)")
            if gst_num_heads not in (2, 4, 8):
                unsupported.append(f"gst_num_heads={gst_num_heads} (2, 4 or 8)")
            if not 1 <= int(gst_style_tokens) <= 32:
                unsupported.append(f"gst_style_tokens={gst_style_tokens} (1 to 32)")
        if attn_type not in ("original", "graves"):
            unsupported.append(f"attn_type={attn_type}")
        if trans_agent and not forward_attn:
            unsupported.append("trans_agent without forward_attn")
        if not location_attn:
            unsupported.append("location_attn=False")
        if prenet_type not in ("original", "bn"):
            unsupported.append(f"prenet_type={prenet_type}")
        if encoder_in_features != 512 or decoder_in_features != 512:  # before the speaker columns
            unsupported.append("non-default encoder/decoder feature sizes")
        if decoder_output_dim != 80 or postnet_output_dim != 80:
            unsupported.append("frame channels != 80")
        if attn_norm not in ("sigmoid", "softmax"):
            raise ValueError("Unknown value for attention norm type")
        if unsupported:
            raise NotImplementedError("tts_amd Tacotron2 does not implement: " + ", ".join(unsupported) +
                                      " (SURVEY.md §8f lists these as next steps)")
        self.num_chars = num_chars
        self.num_speakers = num_speakers
        self.r = r
        self.attn_norm = attn_norm
        self.postnet_output_dim = postnet_output_dim
        self.double_decoder_consistency = double_decoder_consistency
        self.cfg = TacotronConfig(num_chars=num_chars, r=r, attn_norm=attn_norm,
                                  double_decoder_consistency=double_decoder_consistency,
                                  ddc_r=ddc_r if ddc_r is not None else r,
                                  num_speakers=num_speakers, speaker_embedding_dim=speaker_embedding_dim,
                                  prenet_type=prenet_type, attn_type=attn_type, attn_K=attn_K,
                                  bidirectional_decoder=bool(bidirectional_decoder),
                                  # GravesAttention ignores the location-attention options (tacotron2.py:177-188)
                                  windowing=bool(attn_win) and attn_type != "graves",
                                  forward_attn=bool(forward_attn) and attn_type != "graves",
                                  trans_agent=bool(trans_agent) and attn_type != "graves",
                                  forward_attn_mask=bool(forward_attn and forward_attn_mask) and attn_type != "graves",
                                  gst=bool(gst), gst_embedding_dim=int(gst_embedding_dim),
                                  gst_num_heads=int(gst_num_heads), gst_style_tokens=int(gst_style_tokens),
                                  gst_use_speaker_embedding=bool(gst_use_speaker_embedding))
        self.gst = bool(gst)
        self.gst_embedding_dim = int(gst_embedding_dim)
        self.gst_style_tokens = int(gst_style_tokens)
        self.gst_use_speaker_embedding = bool(gst_use_speaker_embedding)
        # models/tacotron2.py:50-58 / tacotron_abstract.py:76-81: a learned table unless the caller
        # gives per-sample embeddings of speaker_embedding_dim
        self.embeddings_per_sample = speaker_embedding_dim is not None
        self.speaker_embedding_dim = self.cfg.spk_dim
        self.decoder = Decoder(r, decoder_output_dim)
        populate(self, tacotron2_spec(self.cfg))

    def _speaker_args(self, speaker_ids, speaker_embeddings, B, dev):
        """Speaker conditioning as the reference takes it (models/tacotron2.py:152-155): ids into
        the learned table, or per-sample embeddings (B, speaker_embedding_dim) / (B, 1, dim)."""
        if self.num_speakers <= 1:  # the reference ignores both arguments here (models/tacotron2.py:152)
            return None, None
        if self.embeddings_per_sample:
            if speaker_embeddings is None:
                raise ValueError("this model takes per-sample speaker_embeddings")
            e = torch.as_tensor(speaker_embeddings).to(dev, torch.float32).reshape(-1, self.speaker_embedding_dim)
            if e.shape[0] == 1 and B > 1:
                e = e.expand(B, -1)
            if e.shape[0] != B:
                raise ValueError("speaker_embeddings must have one row per utterance")
            return None, e.contiguous()
        if speaker_ids is None:
            raise ValueError("multi-speaker model: speaker_ids are required")
        ids = torch.as_tensor(speaker_ids).reshape(-1).to(torch.int64)
        if ids.numel() == 1 and B > 1:
            ids = ids.expand(B)
        if ids.numel() != B:
            raise ValueError("speaker_ids must have one entry per utterance")
        if int(ids.min()) < 0 or int(ids.max()) >= self.num_speakers:
            raise IndexError("speaker id out of range")  # nn.Embedding raises too
        return ids.to(dev).contiguous(), None

    def _style_check(self, style_mel, style_lengths, B):
        """The style argument of one call, checked on the host (before anything asks for the device).
        Returns None (no style: zeros), ("tokens", ids, weights) for a {token: weight} dict, or
        ("mel", mel (Bs, N, 80), lengths) with Bs in (1, B). A mel of any shape is read as the
        reference's ``inputs.view(B, 1, -1, 80)`` reads it (gst_layers.py:63): rows of 80 values of its
        contiguous memory -- synthesis() hands over (1, 80, N), untransposed, and so may a caller."""
        if not self.gst:
            if style_mel is not None:
                raise NotImplementedError("style_mel needs a model built with gst=True (GST style conditioning)")
            if style_lengths is not None:
                raise ValueError("style_lengths without style_mel")
            return None
        if style_mel is None:
            if style_lengths is not None:
                raise ValueError("style_lengths without style_mel")
            return None
        if isinstance(style_mel, dict):
            if style_lengths is not None:
                raise ValueError("style_lengths goes with a style mel, not with a token dict")
            ids, ws = [], []
            for k, v in style_mel.items():
                k = int(k)
                if not -self.gst_style_tokens <= k < self.gst_style_tokens:  # torch indexing: negatives wrap
                    raise IndexError(f"index {k} is out of bounds for dimension 0 with size {self.gst_style_tokens}")
                ids.append(k % self.gst_style_tokens)
                ws.append(float(v))
            if len(ids) > 64:
                raise ValueError("at most 64 token weights")
            return "tokens", ids, ws
        mel = torch.as_tensor(style_mel)
        if mel.dim() < 2 or mel.shape[0] < 1 or mel[0].numel() == 0 or mel[0].numel() % 80 != 0:
            raise ValueError("style_mel must be a (B, N, 80) tensor (or any shape viewable as that) or a token dict")
        mel = mel.contiguous().reshape(mel.shape[0], -1, 80)
        Bs, N = mel.shape[:2]
        if Bs not in (1, B):
            raise ValueError("style_mel must have one row per utterance (or one row for all)")
        lens = row_lengths(style_lengths, Bs, N, "style_lengths")
        return "mel", mel, lens

    def _style_vectors(self, eng, checked, B, spk_emb, dev):
        """(B, gst_embedding_dim) style vectors on the device for ``_style_check``'s result, or None
        (zeros). Caller holds ``eng.lock`` and has synced the weights."""
        if checked is None:
            return None
        G = self.gst_embedding_dim
        if checked[0] == "tokens":
            one = torch.empty(G, device=dev, dtype=torch.float32)
            eng.taco_style_tokens(checked[1], checked[2], one)
            return one[None].expand(B, -1).contiguous()
        _, mel, lens = checked
        mel = mel.to(dev, torch.float32)
        emb = spk_emb if self.cfg.gst_query_speaker_dim else None
        if mel.shape[0] == 1 and B > 1 and emb is not None:  # one mel, but a query per speaker embedding
            mel, lens = mel.expand(B, -1, -1), np.repeat(lens, B)
        out = []
        for b0 in range(0, mel.shape[0], SPEAKER_BATCH_LIMIT):
            b1 = min(mel.shape[0], b0 + SPEAKER_BATCH_LIMIT)
            N = int(lens[b0:b1].max())
            st = torch.empty(b1 - b0, G, device=dev, dtype=torch.float32)
            eng.taco_style_mel(mel[b0:b1, :N].contiguous(), lens[b0:b1],
                               None if emb is None else emb[b0:b1].contiguous(), st)
            out.append(st)
        st = out[0] if len(out) == 1 else torch.cat(out)
        return st.expand(B, -1).contiguous() if st.shape[0] != B else st

    @torch.no_grad()
    def style_embedding(self, style_mel, style_lengths=None, speaker_embeddings=None):
        """The style vectors ``inference`` concatenates for ``style_mel`` (a mel tensor, a token dict
        or None), (rows, gst_embedding_dim): ``gst_layer(style_mel, speaker_embeddings)`` of the
        reference for a tensor. ``speaker_embeddings`` (rows, dim) is needed when the style
        attention's query takes it (``gst_use_speaker_embedding`` with external embeddings)."""
        if not self.gst:
            raise NotImplementedError("style_embedding needs a model built with gst=True")
        rows = 1 if style_mel is None or isinstance(style_mel, dict) else int(torch.as_tensor(style_mel).shape[0])
        checked = self._style_check(style_mel, style_lengths, rows)
        emb = None
        if checked is not None and checked[0] == "mel" and self.cfg.gst_query_speaker_dim:
            if speaker_embeddings is None:
                raise ValueError("this model's style query takes the per-sample speaker_embeddings")
            emb = torch.as_tensor(speaker_embeddings).reshape(-1, self.cfg.gst_query_speaker_dim)
            if emb.shape[0] != rows:
                raise ValueError("speaker_embeddings must have one row per style mel")
        dev = self.device
        eng = self._engine()  # a CPU model stops here: there is no CPU fallback
        if checked is None:
            return torch.zeros(1, self.gst_embedding_dim, device=dev)
        if emb is not None:
            emb = emb.to(dev, torch.float32).contiguous()
        with eng.lock:
            self._sync(eng)
            return self._style_vectors(eng, checked, rows, emb, dev)

    def _load(self, eng):
        eng.load_tacotron(host_tensors(self, skip_prefixes=("coarse_decoder.", "decoder_backward.")), self.num_chars,
                          self.decoder.r_init, self.attn_norm, self.cfg.windowing, self.cfg.forward_attn,
                          self.cfg.forward_attn_mask)

    def _prepare(self, text, speaker_ids, speaker_embeddings, text_lengths, max_decoder_steps):
        """Arguments of one inference call, checked and placed: (device, engine, ids, lengths, per-row
        max steps, r, speaker ids / embeddings, rows per library call)."""
        dev, eng, text, lens, ms, r = self._text_args(text, text_lengths, max_decoder_steps)
        spk_ids, spk_emb = self._speaker_args(speaker_ids, speaker_embeddings, text.shape[0], dev)
        variant = self.cfg.prenet_type == "bn" or self.cfg.windowing or self.cfg.forward_attn or \
            self.cfg.attn_type == "graves"
        limit = BATCH_LIMIT if self.num_speakers <= 1 and not variant else SPEAKER_BATCH_LIMIT
        return dev, eng, text, lens, ms, r, spk_ids, spk_emb, limit

    @torch.no_grad()
    def inference(self, text, speaker_ids=None, style_mel=None, speaker_embeddings=None,
                  text_lengths: Optional[Sequence[int]] = None, max_decoder_steps=None, style_lengths=None):
        """``style_mel`` (models built with ``gst=True``): a mel tensor (B or 1 rows of N frames;
        with ``style_lengths`` row i uses its first N_i frames and equals the reference B = 1 call on
        ``style_mel[i:i+1, :N_i]``), a ``{token: weight}`` dict (one style for all rows) or None (a
        zero style vector), as tacotron_abstract.py:184-203."""
        t = torch.as_tensor(text)
        style = self._style_check(style_mel, style_lengths, 1 if t.dim() == 1 else t.shape[0])
        dev, eng, text, lens, ms, r, spk_ids, spk_emb, limit = self._prepare(
            text, speaker_ids, speaker_embeddings, text_lengths, max_decoder_steps)
        B = text.shape[0]
        outs = []
        with eng.lock:
            self._sync(eng)
            style = self._style_vectors(eng, style, B, spk_emb, dev)
            for b0 in range(0, B, limit):
                b1 = min(B, b0 + limit)
                Tn = int(lens[b0:b1].max())
                sub = text[b0:b1, :Tn].contiguous()
                S_cap = int(ms[b0:b1].max())
                dec, post, align, stop = self._out_tensors(b1 - b0, S_cap, r, Tn, dev)
                steps, status = eng.taco_infer(
                    sub, lens[b0:b1], r, ms[b0:b1], S_cap, self.decoder.stop_threshold, dec, post, align, stop,
                    speaker_ids=None if spk_ids is None else spk_ids[b0:b1].contiguous(),
                    speaker_embeddings=None if spk_emb is None else spk_emb[b0:b1].contiguous(),
                    **({} if style is None else {"style": style[b0:b1].contiguous()}))
                outs.append((dec, post, align, stop, steps, status))
        self._last_call = (B, int(lens.max()), len(outs))
        return self._assemble(outs, text.shape, r, dev)

    @torch.no_grad()
    def forward(self, text, text_lengths, mel_specs=None, mel_lengths=None, speaker_ids=None,
                speaker_embeddings=None):
        """The reference's ``forward`` on a model in ``eval()`` (models/tacotron2.py:95-140,
        layers/tacotron2.py:300-333): the decode driven by the ground-truth ``mel_specs`` (B, M, 80),
        as notebooks/ExtractTTSpectrogram.ipynb calls it for ground-truth-aligned mels and forced
        alignments. Returns (decoder_outputs (B, M, 80), postnet_outputs (B, M, 80), alignments
        (B, M / r, T), stop_tokens (B, M / r), raw stopnet logits).

        Row i equals the reference B = 1 call on that row alone, ``forward(text[i:i+1, :T_i], [T_i],
        mel_specs[i:i+1, :S_i * r], [M_i])`` with ``S_i = ceil(M_i / r)``: it takes S_i steps, and
        everything past its own extent (frames >= M_i, steps >= S_i, positions >= T_i) is zero.
        ``mel_lengths=None``: every row has M frames. ``text_lengths`` need not be sorted. Models
        with ``double_decoder_consistency`` / ``bidirectional_decoder`` return the same 4-tuple (the
        reference adds two training-loss tensors). ``last_steps`` holds S_i, ``last_mel_lengths`` M_i.
        A model with ``gst=True`` takes each row's style from its own teacher mel, as the reference
        does (models/tacotron2.py:103-107): frames [0, M_i) followed by zeros up to S_i r, which is what
        the B = 1 call on the zero-padded row sees.
        Training (``self.training``) stays out of scope."""
        if self.training:
            return super().forward()
        for on, name in ((self.cfg.attn_type == "graves", 'attn_type="graves"'), (self.cfg.windowing, "attn_win"),
                         (self.cfg.forward_attn, "forward_attn")):
            if on:
                raise NotImplementedError(f"tts_amd Tacotron2.forward does not implement {name} (inference() does)")
        if mel_specs is None:
            raise ValueError("forward is teacher-forced: mel_specs (B, M, 80) is required")
        text = torch.as_tensor(text)
        if text.dim() == 1:
            text = text[None]
        mel = torch.as_tensor(mel_specs)
        if mel.dim() != 3 or mel.shape[2] != self.decoder.frame_channels:
            raise ValueError(f"mel_specs must be (B, M, {self.decoder.frame_channels})")
        B, T = text.shape
        if mel.shape[0] != B:
            raise ValueError("mel_specs must have one row per row of text")
        lens = row_lengths(text_lengths, B, T, "text_lengths")
        r = int(self.decoder.r)
        if not 1 <= r <= self.decoder.r_init:
            raise ValueError(f"r={r} must be in [1, r_init={self.decoder.r_init}]")
        M = int(mel.shape[1])
        if M < 1 or M % r != 0:  # the reference's memory.view(B, M // r, -1) (layers/tacotron2.py:241)
            raise RuntimeError(f"shape '[{B}, {M // r}, -1]' is invalid for input of size {mel.numel()}: "
                               f"mel_specs.shape[1] must be a multiple of r={r}")
        mlens = np.full(B, M, np.int64) if mel_lengths is None else \
            np.asarray(torch.as_tensor(mel_lengths).cpu(), dtype=np.int64).reshape(-1)
        if len(mlens) != B or mlens.min() < 1 or mlens.max() > M:
            raise ValueError("mel_lengths must have B entries in [1, M]")
        dev = self.device
        spk_ids, spk_emb = self._speaker_args(speaker_ids, speaker_embeddings, B, dev)
        eng = self._engine()  # a CPU model stops here: there is no CPU fallback
        text = text.to(dev, torch.int64).contiguous()
        mel = mel.to(dev, torch.float32)
        steps = -(-mlens // r)
        S = M // r
        outs = []
        with eng.lock:
            self._sync(eng)
            style = None
            if self.gst:
                frames = torch.arange(M, device=dev)[None, :, None] < torch.as_tensor(mlens, device=dev)[:, None, None]
                smel = torch.where(frames, mel, torch.zeros((), device=dev))
                style = self._style_vectors(eng, ("mel", smel, steps * r), B, spk_emb, dev)
            for b0 in range(0, B, SPEAKER_BATCH_LIMIT):
                b1 = min(B, b0 + SPEAKER_BATCH_LIMIT)
                Tn, Sn = int(lens[b0:b1].max()), int(steps[b0:b1].max())
                dec, post, align, stop = self._out_tensors(b1 - b0, Sn, r, Tn, dev)
                eng.taco_forward(text[b0:b1, :Tn].contiguous(), lens[b0:b1], r, mel[b0:b1, :Sn * r].contiguous(),
                                 mlens[b0:b1], dec, post, align, stop,
                                 speaker_ids=None if spk_ids is None else spk_ids[b0:b1].contiguous(),
                                 speaker_embeddings=None if spk_emb is None else spk_emb[b0:b1].contiguous(),
                                 **({} if style is None else {"style": style[b0:b1].contiguous()}))
                outs.append((dec, post, align, stop))
        if len(outs) == 1 and outs[0][2].shape[1:] == (S, T):
            dec, post, align, stop = outs[0]
        else:  # library calls cover their own longest row: zero-extended to the call's (M, S, T)
            dec = torch.zeros(B, M, 80, device=dev)
            post = torch.zeros(B, M, self.postnet_output_dim, device=dev)
            align = torch.zeros(B, S, T, device=dev)
            stop = torch.zeros(B, S, device=dev)
            b0 = 0
            for d_, p_, a_, s_ in outs:
                n, Sn, Tn = a_.shape
                dec[b0:b0 + n, :Sn * r], post[b0:b0 + n, :Sn * r] = d_, p_
                align[b0:b0 + n, :Sn, :Tn], stop[b0:b0 + n, :Sn] = a_, s_
                b0 += n
        self._last_call = (B, int(lens.max()), len(outs))
        self.last_steps = steps.astype(np.int32)
        self.last_mel_lengths = mlens.astype(np.int32)
        self.last_status = None
        return dec, post, align, stop

    @torch.no_grad()
    def inference_vocoded(self, text, vocoder, speaker_ids=None, speaker_embeddings=None,
                          text_lengths: Optional[Sequence[int]] = None, max_decoder_steps=None, style_mel=None,
                          style_lengths=None):
        """``inference`` followed by ``vocoder.inference(postnet_outputs.transpose(1, 2),
        lengths=last_mel_lengths)`` -- the pair TTS/server/synthesizer.py:150-159 runs -- in one
        library call when ``vocoder`` is a MultibandMelganGenerator on the same device and the batch
        fits one decode (tts_taco_mbmelgan_infer: the vocoder is launched on the decoded lengths the
        decode leaves on the device, no host round trip between the models); otherwise the two
        calls. Returns (decoder_outputs, postnet_outputs, alignments, stop_tokens, waveforms (B, 1,
        hop * (M + 2 pad))), bit-identical to the two calls either way. With ``style_mel`` (GST models) it
        is the two calls: the fused library entry takes no style vector."""
        return self._vocoded(text, vocoder, speaker_ids, speaker_embeddings, text_lengths, max_decoder_steps,
                             submit=False, style_mel=style_mel, style_lengths=style_lengths).result()

    @torch.no_grad()
    def inference_vocoded_submit(self, text, vocoder, speaker_ids=None, speaker_embeddings=None,
                                 text_lengths: Optional[Sequence[int]] = None, max_decoder_steps=None, style_mel=None,
                                 style_lengths=None):
        """``inference_vocoded`` in two halves (tts_taco_mbmelgan_submit / _finish): returns a
        ``VocodedResult`` once the decode is done, with the vocoder still running on the device, so
        that the caller can queue the next batch behind it; ``.result()`` waits for the vocoder
        (re-running it in fp32 if its split-f16 operands left the f16 range) and returns what
        ``inference_vocoded`` returns. The decode outputs (``.outputs[:4]``) are ready at once."""
        return self._vocoded(text, vocoder, speaker_ids, speaker_embeddings, text_lengths, max_decoder_steps,
                             submit=True, style_mel=style_mel, style_lengths=style_lengths)

    def _vocoded(self, text, vocoder, speaker_ids, speaker_embeddings, text_lengths, max_decoder_steps, submit,
                 style_mel=None, style_lengths=None):
        from .vocoder import MultibandMelganGenerator
        if style_mel is not None or style_lengths is not None:
            dec, post, align, stop = self.inference(text, speaker_ids=speaker_ids, style_mel=style_mel,
                                                    speaker_embeddings=speaker_embeddings, text_lengths=text_lengths,
                                                    max_decoder_steps=max_decoder_steps, style_lengths=style_lengths)
            wav = vocoder.inference(post.transpose(1, 2), lengths=self.last_mel_lengths)
            return VocodedResult((dec, post, align, stop), wav)
        dev, eng, text, lens, ms, r, spk_ids, spk_emb, limit = self._prepare(
            text, speaker_ids, speaker_embeddings, text_lengths, max_decoder_steps)
        B = text.shape[0]
        vdev = vocoder.device if isinstance(vocoder, MultibandMelganGenerator) else None
        if vdev != dev or B > limit or vocoder.cfg.in_channels != 80:
            dec, post, align, stop = self.inference(text, speaker_ids=speaker_ids, speaker_embeddings=speaker_embeddings,
                                                    text_lengths=lens, max_decoder_steps=ms)
            wav = vocoder.inference(post.transpose(1, 2), lengths=self.last_mel_lengths)
            return VocodedResult((dec, post, align, stop), wav)
        pad = int(vocoder.inference_padding)
        Tn = int(lens.max())
        sub = text[:, :Tn].contiguous()
        S_cap = int(ms.max())
        dec, post, align, stop = self._out_tensors(B, S_cap, r, Tn, dev)
        hop = vocoder.hop
        wbuf = torch.empty(B * hop * (S_cap * r + 2 * pad), device=dev, dtype=torch.float32)
        with eng.lock:
            self._sync(eng)
            vocoder._sync(eng)
            args = (sub, lens, r, ms, S_cap, self.decoder.stop_threshold, dec, post, align, stop, pad, wbuf)
            if submit:
                steps, status, ticket = eng.taco_mbmelgan_submit(*args, speaker_ids=spk_ids, speaker_embeddings=spk_emb)
            else:
                steps, status = eng.taco_mbmelgan_infer(*args, speaker_ids=spk_ids, speaker_embeddings=spk_emb)
                ticket = None
        self._last_call = (B, Tn, 1)
        res = self._assemble([(dec, post, align, stop, steps, status)], text.shape, r, dev)
        L = hop * (int(steps.max()) * r + 2 * pad)
        return VocodedResult(res, wbuf[:B * L].view(B, 1, L), eng, ticket)

    @torch.no_grad()
    def decoder_state(self):
        """The decoder state the reference leaves on ``self.decoder`` after ``inference`` (query,
        attention_rnn_cell_state, decoder_hidden, decoder_cell, context,
        attention.attention_weights / attention_weights_cum; layers/tacotron2.py:217-233,259-298,
        common_layers.py:251-260), for the last call's rows in caller order: (B, 1024) x 4,
        (B, 512), (B, T) x 2. Rows that stopped before the call's last step hold the batched
        decode's state, not their own final one (the reference decodes B = 1)."""
        B, T, nchunks = getattr(self, "_last_call", (0, 0, 0))
        if not B:
            raise RuntimeError("run inference first")
        if nchunks != 1:
            raise RuntimeError("decoder_state: the last call was split into several library calls")
        return self._engine().taco_decoder_state(B, T, self.device, key=self.weight_key)
