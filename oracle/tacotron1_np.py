"""ORACLE (test infrastructure only): numpy restatement of the reference Tacotron (v1) inference
path for the single-speaker model, in float64 by default. Only ``tests/`` may import this module;
nothing under ``tts_amd/`` and nothing in ``bench.py`` does.

Parity pin: ``tests/test_tacotron1_oracle.py`` checks it against ``tests/golden/tacotron1_f64.npz``
(the reference run in float64, ``tests/golden/make_tacotron1_golden.py f64``) and against the float32
fixtures ``tests/golden/tacotron1_*.npz``.

Every function follows one reference op sequence, cited file:line (paths relative to the reference
checkout):

* ``TTS/tts/models/tacotron.py:150-172``       Tacotron.inference
* ``TTS/tts/layers/tacotron.py:7-66``          BatchNormConv1d (pad -> conv -> BN(eval, eps 1e-3) -> act)
* ``TTS/tts/layers/tacotron.py:69-101``        Highway
* ``TTS/tts/layers/tacotron.py:104-205``       CBHG (bank, projections, residual, highways, BiGRU);
  the reference's CBHG concatenates the bank outputs and has no max-pool between bank and projections
* ``TTS/tts/layers/tacotron.py:226-261``       Encoder, PostCBHG
* ``TTS/tts/layers/tacotron.py:353-371``       Decoder._init_states
* ``TTS/tts/layers/tacotron.py:383-414``       Decoder.decode
* ``TTS/tts/layers/tacotron.py:416-430``       Decoder._update_memory_input
* ``TTS/tts/layers/tacotron.py:465-495``       Decoder.inference (AR loop, stop rule :489-494)
* ``TTS/tts/layers/common_layers.py:76-82``    Prenet.forward (eval: no dropout)
* ``TTS/tts/layers/common_layers.py:90-110``   LocationLayer
* ``TTS/tts/layers/common_layers.py:268-278,325-372`` OriginalAttention (location-sensitive, norm)

``dtype=np.float32`` evaluates the same op sequence in float32: the distance between the two is the
yardstick ("e32") for what a correct float32 implementation may differ by.

``hook(name, array)`` is called on a few intermediates and may return a replacement (None keeps the
value); the sensitivity tests perturb one element through it:

* ``"memory"``   the memory input entering the decoder prenet, every step
* ``"align"``    the alignment as the context sum reads it (a replacement changes the context only;
  the attention state and the returned alignment keep the unperturbed value)
* ``"context"``  the context vector
"""

import numpy as np


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-x))


def _conv1d(x, w, pad):
    """x (Cin, L), w (Cout, Cin, K), zero padding (left, right) -> (Cout, L + left + right - K + 1)."""
    cin, L = x.shape
    cout, _, K = w.shape
    xp = np.pad(x, ((0, 0), pad))
    Lout = xp.shape[1] - K + 1
    cols = np.empty((cin, K, Lout), x.dtype)
    for k in range(K):
        cols[:, k, :] = xp[:, k:k + Lout]
    return w.reshape(cout, cin * K) @ cols.reshape(cin * K, Lout)


class Tacotron1Oracle:
    def __init__(self, sd, cfg, dtype=np.float64, hook=None):
        """sd: the reference's state dict (name -> array), cfg: a ``TacotronV1Config``."""
        self.dtype = np.dtype(dtype)
        self.sd = {k: np.asarray(v).astype(self.dtype) for k, v in sd.items()
                   if not k.endswith("num_batches_tracked")}
        self.cfg = cfg
        self.F = cfg.frame_channels
        self.r_init = cfg.r
        self.use_memory_queue = cfg.memory_size > 0
        self.memory_size = cfg.memory_size if cfg.memory_size > 0 else cfg.r  # layers/tacotron.py:300-301
        self.hook = hook

    def _hooked(self, name, x):
        if self.hook is None:
            return x
        y = self.hook(name, x)
        return x if y is None else np.asarray(y, self.dtype)

    def _linear(self, name, x, bias=True):
        y = x @ self.sd[name + ".weight"].T
        return y + self.sd[name + ".bias"] if bias else y

    # ---- CBHG ----------------------------------------------------------------------------------
    def bn_conv(self, prefix, x, pad, relu):
        """BatchNormConv1d.forward (layers/tacotron.py:60-66), BatchNorm1d in eval mode, eps 1e-3."""
        sd = self.sd
        y = _conv1d(x, sd[prefix + ".conv1d.weight"], pad)
        inv = 1 / np.sqrt(sd[prefix + ".bn.running_var"] + self.dtype.type(1e-3))
        y = (y - sd[prefix + ".bn.running_mean"][:, None]) * inv[:, None] * sd[prefix + ".bn.weight"][:, None] \
            + sd[prefix + ".bn.bias"][:, None]
        return np.maximum(y, 0) if relu else y

    def gru_cell(self, prefix, sfx, x, h):
        """torch.nn.GRUCell / one nn.GRU step: gates r, z, n (chunk order)."""
        sd = self.sd
        gi = x @ sd[f"{prefix}.weight_ih{sfx}"].T + sd[f"{prefix}.bias_ih{sfx}"]
        gh = h @ sd[f"{prefix}.weight_hh{sfx}"].T + sd[f"{prefix}.bias_hh{sfx}"]
        H = h.shape[-1]
        r = _sigmoid(gi[:H] + gh[:H])
        z = _sigmoid(gi[H:2 * H] + gh[H:2 * H])
        n = np.tanh(gi[2 * H:] + r * gh[2 * H:])
        return (1 - z) * n + z * h

    def cbhg(self, prefix, x, K):
        """CBHG.forward (layers/tacotron.py:179-205); x (C, T) -> (T, 256)."""
        sd = self.sd
        inputs = x
        x = np.concatenate([self.bn_conv(f"{prefix}.conv1d_banks.{k - 1}", inputs, ((k - 1) // 2, k // 2), True)
                            for k in range(1, K + 1)], axis=0)                      # :185-188
        x = self.bn_conv(f"{prefix}.conv1d_projections.0", x, (1, 1), True)        # :190-191
        x = self.bn_conv(f"{prefix}.conv1d_projections.1", x, (1, 1), False)
        x = (x + inputs).T                                                         # :192-193
        if f"{prefix}.pre_highway.weight" in sd:                                   # :194-195
            x = x @ sd[f"{prefix}.pre_highway.weight"].T
        for i in range(4):                                                         # Highway.forward :98-101
            H = np.maximum(self._linear(f"{prefix}.highways.{i}.H", x), 0)
            T = _sigmoid(self._linear(f"{prefix}.highways.{i}.T", x))
            x = H * T + x * (1 - T)
        n = x.shape[0]
        out = np.zeros((n, 256), self.dtype)                                       # nn.GRU, bidirectional
        for d, (sfx, order) in enumerate((("_l0", range(n)), ("_l0_reverse", range(n - 1, -1, -1)))):
            h = np.zeros(128, self.dtype)
            for t in order:
                h = self.gru_cell(f"{prefix}.gru", sfx, x[t], h)
                out[t, d * 128:(d + 1) * 128] = h
        return out

    def _prenet(self, prefix, x):
        """Prenet.forward (common_layers.py:76-82), 'original' type with bias, eval mode."""
        for i in range(2):
            x = np.maximum(self._linear(f"{prefix}.linear_layers.{i}.linear_layer", x), 0)
        return x

    def encoder(self, ids):
        """embedding (models/tacotron.py:152) + Encoder.forward (layers/tacotron.py:241-245) -> (T, 256)."""
        x = self.sd["embedding.weight"][np.asarray(ids)]
        x = self._prenet("encoder.prenet", x)
        return self.cbhg("encoder.cbhg.cbhg", x.T, 16)

    def postnet(self, dec):
        """PostCBHG + last_linear (models/tacotron.py:169-170); dec (M, 80) -> (M, postnet_output_dim)."""
        x = self.cbhg("postnet.cbhg", np.asarray(dec, self.dtype).T, 8)
        return self._linear("last_linear", x)

    # ---- decoder -------------------------------------------------------------------------------
    def attention(self, query, inputs, pin, st):
        """OriginalAttention.forward (common_layers.py:325-372) with location attention, mask None."""
        sd, p = self.sd, "decoder.attention."
        cat = np.stack([st["alpha"], st["alpha_cum"]])                              # :269-271
        pq = query @ sd[p + "query_layer.linear_layer.weight"].T
        f = _conv1d(cat, sd[p + "location_layer.location_conv1d.weight"], (15, 15))  # LocationLayer :106-110
        loc = f.T @ sd[p + "location_layer.location_dense.linear_layer.weight"].T
        e = np.tanh(pq[None, :] + loc + pin) @ sd[p + "v.linear_layer.weight"][0] + sd[p + "v.linear_layer.bias"][0]
        if self.cfg.attn_norm == "softmax":                                         # :347-352
            z = np.exp(e - e.max())
            a = z / z.sum()
        elif self.cfg.attn_norm == "sigmoid":
            s = _sigmoid(e)
            a = s / s.sum()
        else:
            raise ValueError("Unknown value for attention norm type")
        st["alpha_cum"] = st["alpha_cum"] + a                                       # :356-357
        st["alpha"] = a
        return self._hooked("context", self._hooked("align", a) @ inputs)           # :364-365

    def decode(self, inputs, pin, st):
        """Decoder.decode (layers/tacotron.py:383-414) -> (all r_init frames, stop logit)."""
        m = self._prenet("decoder.prenet", self._hooked("memory", st["memory"]))
        st["q"] = self.gru_cell("decoder.attention_rnn", "", np.concatenate([m, st["ctx"]]), st["q"])
        st["ctx"] = self.attention(st["q"], inputs, pin, st)
        d = self._linear("decoder.project_to_decoder_in", np.concatenate([st["q"], st["ctx"]]))
        for i in range(2):
            st["h"][i] = self.gru_cell(f"decoder.decoder_rnns.{i}", "", d, st["h"][i])
            d = st["h"][i] + d
        y = self._linear("decoder.proj_to_mel", d)
        logit = self._linear("decoder.stopnet.linear", np.concatenate([d, y]))[0]
        return y, logit

    def update_memory(self, st, new, r):
        """Decoder._update_memory_input (layers/tacotron.py:416-430); new: the r frames just emitted."""
        F = self.F
        if self.use_memory_queue:
            if self.memory_size > r:
                st["memory"] = np.concatenate([new, st["memory"][:(self.memory_size - r) * F]])
            else:
                st["memory"] = new[:self.memory_size * F]
        else:
            st["memory"] = new[F * (r - 1):]

    def decoder_inference(self, inputs, r, max_steps):
        """Decoder.inference (layers/tacotron.py:465-495) at B = 1."""
        F, dt = self.F, self.dtype
        T = inputs.shape[0]
        st = dict(memory=np.zeros(F * self.memory_size if self.use_memory_queue else F, dt),  # :359-362
                  q=np.zeros(256, dt), h=[np.zeros(256, dt), np.zeros(256, dt)], ctx=np.zeros(inputs.shape[1], dt),
                  alpha=np.zeros(T, dt), alpha_cum=np.zeros(T, dt))
        pin = inputs @ self.sd["decoder.attention.inputs_layer.linear_layer.weight"].T  # preprocess_inputs
        outs, aligns, stops, logits, t, status = [], [], [], [], 0, 0
        while True:
            if t > 0:
                self.update_memory(st, outs[-1], r)
            y, lg = self.decode(inputs, pin, st)
            stop = _sigmoid(lg)
            outs.append(y[:r * F])
            aligns.append(st["alpha"])
            stops.append(stop)
            logits.append(lg)
            t += 1
            if t > T / 4 and (stop > 0.6 or st["alpha"][-1] > 0.6):                 # :489-491
                status = 1
                break
            if t > max_steps:                                                       # :492-494
                status = 2
                break
        dec = np.stack(outs).reshape(-1, F)
        return dec, np.stack(aligns), np.array(stops, dt), np.array(logits, dt), t, status

    def inference(self, ids, r, max_steps):
        """Tacotron.inference (models/tacotron.py:150-172) for one utterance: (dec (S r, 80),
        post (S r, postnet_output_dim), align (S, T), stop (S,), raw stop logits (S,), steps S,
        status 1 = stop rule / 2 = max_decoder_steps)."""
        if not 1 <= r <= self.r_init:
            raise ValueError(f"r={r} must be in [1, r_init={self.r_init}]")
        enc = self.encoder(ids)
        dec, align, stop, logits, steps, status = self.decoder_inference(enc, r, max_steps)
        return dec, self.postnet(dec), align, stop, logits, steps, status
