"""The host path ``Tacotron`` and ``Tacotron2`` share: argument handling on the text side and the
assembly of the library calls' outputs into the reference's return values."""

import numpy as np
import torch

from .params import NativeModel, row_lengths


class TacotronHost(NativeModel):
    """Expects ``self.decoder`` (r, r_init, max_decoder_steps) and ``self.postnet_output_dim``."""

    def __init__(self):
        super().__init__()
        self.last_steps = None
        self.last_mel_lengths = None
        self.last_status = None

    def forward(self, *args, **kwargs):
        raise NotImplementedError("training forward is out of scope; use inference()")

    def _text_args(self, text, text_lengths, max_decoder_steps):
        """Text-side arguments of one call, checked and placed: (device, engine, ids (B, T) int64,
        lengths, per-row max steps, r)."""
        dev = self.device
        eng = self._engine()
        text = torch.as_tensor(text).to(dev, torch.int64)
        if text.dim() == 1:
            text = text[None]
        text = text.contiguous()
        B, T = text.shape
        lens = row_lengths(text_lengths, B, T, "text_lengths")
        ms = self.decoder.max_decoder_steps if max_decoder_steps is None else max_decoder_steps
        ms = np.broadcast_to(np.asarray(ms, dtype=np.int64), (B,)).copy()
        r = int(self.decoder.r)
        if not 1 <= r <= self.decoder.r_init:
            raise ValueError(f"r={r} must be in [1, r_init={self.decoder.r_init}]")
        return dev, eng, text, lens, ms, r

    def _out_tensors(self, nb, S_cap, r, Tn, dev):
        dec = torch.empty(nb, S_cap * r, 80, device=dev, dtype=torch.float32)
        return (dec, torch.empty(nb, S_cap * r, self.postnet_output_dim, device=dev, dtype=torch.float32),
                torch.empty(nb, S_cap, Tn, device=dev, dtype=torch.float32),
                torch.empty(nb, S_cap, device=dev, dtype=torch.float32))

    def _assemble(self, outs, shape, r, dev):
        """The library calls' outputs (dec, post, align, stop, steps, status per chunk) as the
        reference's (B, M, 80), (B, M, postnet_output_dim), (B, S, T), (B, S, 1), and the per-row
        lengths on ``self`` (last_steps, last_mel_lengths, last_status)."""
        B, T = shape
        steps = np.concatenate([o[4] for o in outs])
        status = np.concatenate([o[5] for o in outs])
        # reference behaviour (layers/tacotron2.py:365, layers/tacotron.py:493); bench.py mutes it
        if getattr(self.decoder, "verbose", True):
            for s in status:
                if s == 2:
                    print("   | > Decoder stopped with 'max_decoder_steps")
        S = int(steps.max())
        M = S * r
        if len(outs) == 1:
            dec, post, align, stop = outs[0][0][:, :M], outs[0][1][:, :M], outs[0][2][:, :S], outs[0][3][:, :S]
            if align.shape[2] != T:
                align = torch.nn.functional.pad(align, (0, T - align.shape[2]))
        else:
            # chunks of a split batch decode to their own S_cap; each is cut or zero-padded to the
            # batch's S steps (M frames) before joining (a chunk's rows are zero past their own steps)
            dec = torch.zeros(B, M, 80, device=dev)
            post = torch.zeros(B, M, self.postnet_output_dim, device=dev)
            align = torch.zeros(B, S, T, device=dev)
            stop = torch.zeros(B, S, device=dev)
            b0 = 0
            for o in outs:
                n, Sc, Tn = o[2].shape
                s_ = min(S, Sc)
                dec[b0:b0 + n, :s_ * r] = o[0][:, :s_ * r]
                post[b0:b0 + n, :s_ * r] = o[1][:, :s_ * r]
                align[b0:b0 + n, :s_, :Tn] = o[2][:, :s_]
                stop[b0:b0 + n, :s_] = o[3][:, :s_]
                b0 += n
        self.last_steps = steps
        self.last_mel_lengths = steps * r
        self.last_status = status
        return dec, post, align, stop[:, :, None]
