"""Drop-in GE2E ``SpeakerEncoder`` whose ``inference`` runs on MI355X through ``libttship.so``.

Mirrors ``TTS/speaker_encoder/model.py``: the constructor signature (``:31-47``), the checkpoint
keys (``layers.{i}.lstm.*`` / ``layers.{i}.linear.weight`` with projection, ``layers.lstm.*`` /
``layers.linear.*`` without), ``inference(x)`` (``:62-68``: B x T x D mel frames -> B x proj_dim
L2-normalised embedding of the last frame) and ``compute_embedding(x, num_frames, overlap)``
(``:70-88``: the mean of the window embeddings). The windows of one utterance run as ONE batched
call (each window is its own sequence with its own length), not one call per window.

Batching (new, optional): ``inference`` takes per-sequence ``lengths``; row b's embedding is taken
at frame ``lengths[b] - 1`` and equals the reference run on ``x[b:b+1, :lengths[b]]``.
``compute_embedding_batch`` is ``compute_embedding`` for B utterances at once (the counterpart of
``batch_compute_embedding``, ``:91-111``, with every utterance cut by its own length), and
``embed_utterances`` starts from device waveforms.
"""

from typing import Optional, Sequence

import torch

from .params import NativeModel, host_tensors, populate, row_lengths
from .spec import Ge2eConfig, ge2e_spec

MAX_SEQS = 64  # sequences per library call


class SpeakerEncoder(NativeModel):
    _slot = "ge2e"

    def __init__(self, input_dim, proj_dim=256, lstm_dim=768, num_lstm_layers=3, use_lstm_with_projection=True):
        super().__init__()
        if lstm_dim != 768:
            raise NotImplementedError("lstm_dim must be 768 (the reference config; the HIP LSTM is built for it)")
        self.use_lstm_with_projection = use_lstm_with_projection
        self.cfg = Ge2eConfig(input_dim=input_dim, proj_dim=proj_dim, lstm_dim=lstm_dim,
                              num_lstm_layers=num_lstm_layers, use_lstm_with_projection=use_lstm_with_projection)
        populate(self, ge2e_spec(self.cfg))

    def forward(self, x):
        return self.inference(x)

    def _load(self, eng):
        c = self.cfg
        eng.load_ge2e(host_tensors(self), c.input_dim, c.proj_dim, c.lstm_dim, c.num_lstm_layers,
                      c.use_lstm_with_projection)

    @torch.no_grad()
    def inference(self, x, lengths: Optional[Sequence[int]] = None):
        dev = self.device
        eng = self._engine()
        x = torch.as_tensor(x).to(dev, torch.float32)
        if x.dim() == 2:
            x = x[None]
        x = x.contiguous()
        B, T, D = x.shape
        if D != self.cfg.input_dim:
            raise ValueError(f"expected {self.cfg.input_dim} mel channels, got {D}")
        lens = row_lengths(lengths, B, T, "lengths")
        out = torch.empty(B, self.cfg.proj_dim, device=dev)
        with eng.lock:
            self._sync(eng)
            for b0 in range(0, B, MAX_SEQS):
                b1 = min(B, b0 + MAX_SEQS)
                Tn = int(lens[b0:b1].max())
                eng.ge2e_infer(x[b0:b1, :Tn].contiguous(), lens[b0:b1], out[b0:b1])
        return out

    @torch.no_grad()
    def compute_embedding(self, x, num_frames=160, overlap=0.5):
        """Mean of the window embeddings of x (1 x T x D), windows as in model.py:70-88."""
        x = torch.as_tensor(x)
        if x.dim() == 2:
            x = x[None]
        num_overlap = int(num_frames * overlap)
        T = x.shape[1]
        starts = list(range(0, T, num_frames - num_overlap))
        wins = [(o, min(T, o + num_frames)) for o in starts]
        L = max(e - o for o, e in wins)
        batch = torch.zeros(len(wins), L, x.shape[2], dtype=torch.float32, device=x.device)
        for i, (o, e) in enumerate(wins):
            batch[i, :e - o] = x[0, o:e]
        emb = self.inference(batch, lengths=[e - o for o, e in wins])
        return (emb.sum(0, keepdim=True) / len(wins))

    @staticmethod
    def embedding_windows(T, num_frames=160, overlap=0.5):
        """The (offset, end) frame windows `compute_embedding` cuts from T frames (model.py:72-89)."""
        num_overlap = int(num_frames * overlap)
        return [(o, min(T, o + num_frames)) for o in range(0, T, num_frames - num_overlap)]

    @torch.no_grad()
    def compute_embedding_batch(self, mels, lengths, num_frames=160, overlap=0.5):
        """`compute_embedding` of B utterances at once: ``mels`` (B, T_max, D) frame-major, row b
        valid for ``lengths[b]`` frames. The windows of every utterance (ragged at each tail) are
        packed into as few library calls as MAX_SEQS allows, and the per-utterance means are taken
        on the device. Returns (B, proj_dim), usable as ``Tacotron2.inference(speaker_embeddings=)``."""
        dev = self.device
        mels = torch.as_tensor(mels).to(dev, torch.float32)
        B, T_max, D = mels.shape
        lengths = [int(n) for n in lengths]
        if len(lengths) != B or min(lengths) < 1 or max(lengths) > T_max:
            raise ValueError("lengths must have B entries in [1, T_max]")
        wins = [(b, o, e) for b, n in enumerate(lengths) for o, e in self.embedding_windows(n, num_frames, overlap)]
        L = max(e - o for _, o, e in wins)
        # one gather builds every window: frame t of window w is mels[b_w, o_w + t], clamped into the
        # row (frames past a window's own length are never read by the library)
        row = torch.tensor([b for b, _, _ in wins], device=dev)
        off = torch.tensor([o for _, o, _ in wins], device=dev)
        t = (off[:, None] + torch.arange(L, device=dev)[None, :]).clamp_(max=T_max - 1)
        batch = mels[row[:, None], t]
        emb = self.inference(batch, lengths=[e - o for _, o, e in wins])
        # an utterance's windows are consecutive rows of emb: its mean as compute_embedding takes it
        counts = [sum(1 for b2, _, _ in wins if b2 == b) for b in range(B)]
        out, w0 = torch.empty(B, self.cfg.proj_dim, device=dev), 0
        for b, n in enumerate(counts):
            out[b] = emb[w0:w0 + n].sum(0) / n
            w0 += n
        return out

    @torch.no_grad()
    def embed_utterances(self, wavs, lengths, ap):
        """Waveforms (B, L_max) on the device, ``lengths[b]`` samples each -> (B, proj_dim)
        embeddings: ``ap.melspectrogram_batch`` then `compute_embedding_batch`, no host copy between."""
        mels, frames = ap.melspectrogram_batch(wavs, lengths)
        return self.compute_embedding_batch(mels, frames)
