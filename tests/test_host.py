"""CPU: host-side logic of the drop-in boundary (no GPU, no library compute calls)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from tts_amd import (MultibandMelganGenerator, Tacotron2, load_config, setup_generator,  # noqa: F401
                     setup_model)
from tts_amd.spec import MelganConfig, TacotronConfig, tacotron2_spec
from tts_amd.weights import splitmix64_uniform, synth_state_dict
from tts_amd.workload import forced_steps, lj_profile, lpt_shards, pad_batch, replicated_workload, synthetic_ids


def _keys(sd):
    return {k: (tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in sd.items()}


def _ref_keys(name):
    d = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))
    return {k: (tuple(s), t) for k, s, t in d[name]}


def test_tacotron2_state_dict_keys_match_reference_checkpoint():
    m = Tacotron2(num_chars=129, num_speakers=0, r=7, attn_norm="sigmoid", double_decoder_consistency=True, ddc_r=7)
    assert _keys(m.state_dict()) == _ref_keys("tacotron2_ddc")


def test_mbmelgan_state_dict_keys_match_reference_checkpoint():
    v = MultibandMelganGenerator(upsample_factors=(8, 4, 2), num_res_blocks=4)
    assert _keys(v.state_dict()) == _ref_keys("multiband_melgan")
    v.remove_weight_norm()
    assert _keys(v.state_dict()) == _ref_keys("multiband_melgan_wn_removed")


def test_remove_weight_norm_matches_definition():
    cfg = MelganConfig()
    v = MultibandMelganGenerator(upsample_factors=cfg.upsample_factors, num_res_blocks=cfg.num_res_blocks)
    from helpers import melgan_state_dict
    _, sd = melgan_state_dict(7)
    full = v.state_dict()
    for k, t in sd.items():
        full[k] = torch.from_numpy(t)
    v.load_state_dict(full)
    g, vv = sd["layers.3.weight_g"], sd["layers.3.weight_v"]
    v.remove_weight_norm()
    w = v.state_dict()["layers.3.weight"].numpy()
    ref = vv / np.sqrt((vv.astype(np.float64) ** 2).sum(axis=(1, 2), keepdims=True)) * g
    assert np.abs(w - ref).max() <= 1e-6


def test_synthetic_weights_are_version_stable():
    u = splitmix64_uniform(12345, 8)
    assert np.all((u >= -1) & (u < 1))
    sd = synth_state_dict(tacotron2_spec(TacotronConfig()), 0)
    h = hashlib.sha256(sd["decoder.decoder_rnn.weight_hh"].tobytes()).hexdigest()
    again = synth_state_dict(tacotron2_spec(TacotronConfig()), 0)["decoder.decoder_rnn.weight_hh"]
    assert hashlib.sha256(again.tobytes()).hexdigest() == h
    assert sd["decoder.decoder_rnn.weight_hh"].dtype == np.float32


def test_multispeaker_state_dict_keys_and_shapes():
    """models/tacotron2.py:50-58: a learned (num_speakers, 512) table, decoder_in_features 1024;
    per-sample embeddings (tacotron_abstract.py:76-81): no table, 512 + speaker_embedding_dim."""
    m = Tacotron2(num_chars=129, num_speakers=4, double_decoder_consistency=True, ddc_r=7)
    sd = m.state_dict()
    assert tuple(sd["speaker_embedding.weight"].shape) == (4, 512)
    assert tuple(sd["decoder.attention.inputs_layer.linear_layer.weight"].shape) == (128, 1024)
    assert tuple(sd["decoder.linear_projection.linear_layer.weight"].shape) == (560, 2048)
    assert tuple(sd["coarse_decoder.decoder_rnn.weight_ih"].shape) == (4096, 2048)
    m2 = Tacotron2(num_chars=129, num_speakers=2, speaker_embedding_dim=256)
    sd2 = m2.state_dict()
    assert "speaker_embedding.weight" not in sd2
    assert tuple(sd2["decoder.attention_rnn.weight_ih"].shape) == (4096, 256 + 768)


# (Graves attention with speaker embeddings is supported since round 3: test_gpu_parity graves_spk)
@pytest.mark.parametrize("kw", [dict(gst=True), dict(trans_agent=True), dict(prenet_type="xyz"),
                                dict(location_attn=False)])
def test_unsupported_tacotron_variants_raise(kw):
    with pytest.raises(NotImplementedError):
        Tacotron2(num_chars=129, **kw)


def test_unknown_attention_norm_raises_valueerror():
    with pytest.raises(ValueError):
        Tacotron2(num_chars=129, attn_norm="entmax")


def test_no_cpu_fallback():
    m = Tacotron2(num_chars=129, r=2, attn_norm="sigmoid")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(torch.ones(1, 5, dtype=torch.long))
    v = MultibandMelganGenerator(upsample_factors=(8, 4, 2), num_res_blocks=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.inference(torch.zeros(1, 80, 8))


def test_decoder_knobs():
    m = Tacotron2(num_chars=129, r=7, attn_norm="sigmoid")
    assert m.decoder.max_decoder_steps == 1000 and m.decoder.r == 7 and m.decoder.stop_threshold == 0.5
    m.decoder.set_r(2)
    m.decoder.max_decoder_steps = 3000
    assert m.decoder.r == 2 and m.decoder.r_init == 7


CONFIG_TTS = """{
  // Tacotron2-DDC style config (comments are stripped like TTS/utils/io.py:20-34)
  "model": "Tacotron2",
  "r": 7,
  "audio": {"num_mels": 80, "fft_size": 1024, "sample_rate": 22050},
  "use_gst": false,
  "gst": {"gst_embedding_dim": 512, "gst_num_heads": 4, "gst_style_tokens": 10, "gst_use_speaker_embedding": false},
  "attention_type": "original", "attention_heads": 4, "attention_norm": "sigmoid", "windowing": false,
  "prenet_type": "original", "prenet_dropout": false, "use_forward_attn": false, "transition_agent": false,
  "forward_attn_mask": false, "location_attn": true, "separate_stopnet": true,
  "bidirectional_decoder": false, "double_decoder_consistency": true, "ddc_r": 7
}
"""

CONFIG_VOC = """{
  "audio": {"num_mels": 80},
  "generator_model": "multiband_melgan_generator",  // MB-MelGAN
  "generator_model_params": {"upsample_factors": [8, 4, 2], "num_res_blocks": 4}
}
"""


def test_factories_build_drop_in_models(tmp_path):
    p = tmp_path / "config.json"
    p.write_text(CONFIG_TTS)
    c = load_config(str(p))
    assert c.model == "Tacotron2" and c.attention_norm == "sigmoid"
    m = setup_model(129, 0, c)
    assert isinstance(m, Tacotron2) and m.decoder.r_init == 7 and m.attn_norm == "sigmoid"
    assert _keys(m.state_dict()) == _ref_keys("tacotron2_ddc")
    q = tmp_path / "vocoder.json"
    q.write_text(CONFIG_VOC)
    v = setup_generator(load_config(str(q)))
    assert isinstance(v, MultibandMelganGenerator) and v.hop == 256
    assert _keys(v.state_dict()) == _ref_keys("multiband_melgan")


def test_lj_profile_and_workload():
    T, M = lj_profile()
    assert len(T) == 32 and sum(T) == 3346 and sum(M) == 19112 and max(T) == 168 and max(M) == 857
    steps = forced_steps(M, 2)
    assert all(s * 2 >= m > (s - 1) * 2 for s, m in zip(steps, M))
    ids = synthetic_ids(T)
    assert [len(x) for x in ids] == T and min(x.min() for x in ids) >= 1 and max(x.max() for x in ids) <= 128
    batch, lens = pad_batch(ids[:3])
    assert batch.shape == (3, max(T[:3])) and list(lens) == T[:3]
    assert (batch[0, lens[0]:] == 0).all()


def test_lpt_shards_partition_and_balance():
    T, M = lj_profile()
    costs = forced_steps(M, 2)
    for n in (1, 2, 4, 8):
        sh = lpt_shards(costs, n)
        flat = sorted(i for s in sh for i in s)
        assert flat == list(range(len(costs)))
        assert max(len(s) for s in sh) - min(len(s) for s in sh) <= 1
        loads = [sum(costs[i] for i in s) for s in sh]
        assert max(loads) - min(loads) <= max(costs)


def test_replicated_workload_weak_scaling():
    for n in (1, 2, 4, 8):
        T, M, shards = replicated_workload(n, 32)
        assert len(shards) == n and all(len(s) == 32 for s in shards)
        assert sorted(i for s in shards for i in s) == list(range(32 * n))
        assert sum(M[i] for i in shards[-1]) == 19112
        # bench.py's plan (tts_amd.multigpu.shard_plan, LPT on the step counts) gives every rank one
        # copy of each profile utterance: the per-rank work of C2
        from tts_amd.multigpu import shard_plan
        plan = shard_plan([s_ * 1e6 + t_ for s_, t_ in zip(forced_steps(M, 2), T)], n)
        assert all(sorted(i % 32 for i in s) == list(range(32)) for s in plan)


def test_glow_tts_constructor_and_keys():
    """glow_tts.py:17-95 with the gated-conv encoder: checkpoint key layout; other encoders raise."""
    from tts_amd import GlowTts
    m = GlowTts(num_chars=130)
    sd = m.state_dict()
    assert tuple(sd["encoder.emb.weight"].shape) == (130, 192)
    assert tuple(sd["encoder.proj_m.weight"].shape) == (80, 192, 1)
    assert tuple(sd["decoder.flows.1.weight"].shape) == (4, 4)
    assert m.noise_scale == 0.66 and m.length_scale == 1.
    for kw in (dict(encoder_type="transformer", rel_attn_window_size=4, use_encoder_prenet=True),
               dict(encoder_type="transformer"), dict(mean_only=False)):
        with pytest.raises(NotImplementedError):
            GlowTts(num_chars=130, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.inference(torch.ones(1, 5, dtype=torch.long), [5])


def test_glow_tts_multispeaker_keys_and_misuse():
    """Multi-speaker GlowTts (glow_tts.py:97-99, encoder.py:112-114, glow.py:87-91): emb_g, the
    duration predictor's hidden + c_in inputs, one weight-normed cond_layer per coupling block, in
    the reference's key order (pinned against the reference module by make_golden.py glow_spk); g
    misuse fails before any GPU work, with the reference's exception types."""
    from tts_amd import GlowTts
    m = GlowTts(num_chars=130, num_speakers=4, c_in_channels=36)
    sd = m.state_dict()
    keys = list(sd)
    assert keys[-1] == "emb_g.weight" and tuple(sd["emb_g.weight"].shape) == (4, 36)
    assert tuple(sd["encoder.duration_predictor.conv_1.weight"].shape) == (256, 192 + 36, 3)
    assert tuple(sd["decoder.flows.2.wn.cond_layer.weight_v"].shape) == (2 * 192 * 4, 36, 1)
    assert keys.index("decoder.flows.2.wn.cond_layer.bias") == keys.index("decoder.flows.2.wn.res_skip_layers.3.weight_v") + 1
    assert sum(k.endswith("cond_layer.weight_g") for k in keys) == 12
    x = torch.ones(1, 5, dtype=torch.long)
    with pytest.raises(RuntimeError, match="pass g"):
        m.inference(x, [5])
    with pytest.raises(IndexError):
        m.inference(x, [5], g=torch.tensor([4]))
    with pytest.raises(AttributeError, match="emb_g"):
        GlowTts(num_chars=130).inference(x, [5], g=torch.tensor([0]))
    # setup_model's multi-speaker call (num_speakers > 1, c_in_channels = 0): an empty emb_g, and g
    # cannot reach a cond_layer
    m0 = GlowTts(num_chars=130, num_speakers=4)
    assert tuple(m0.state_dict()["emb_g.weight"].shape) == (4, 0)
    with pytest.raises(AttributeError, match="cond_layer"):
        m0.inference(x, [5], g=torch.tensor([0]))


def test_pwgan_keys_match_reference_and_factory():
    """parallel_wavegan_generator.py:16-88 checkpoint keys (pinned against the reference module by
    make_golden.py pwgan), remove_weight_norm folding, setup_generator dispatch."""
    from tts_amd import ParallelWaveganGenerator
    from tts_amd.spec import PwganConfig, pwgan_spec
    g = ParallelWaveganGenerator()
    assert [(k, tuple(v.shape)) for k, v in g.state_dict().items()] == \
        [(n, tuple(s)) for n, s, _ in pwgan_spec(PwganConfig())]
    assert tuple(g.state_dict()["upsample_net.upsample.up_layers.7.weight_v"].shape) == (1, 1, 1, 9)
    g.remove_weight_norm()
    sd = g.state_dict()
    assert "conv_layers.29.conv.weight" in sd and "conv_layers.29.conv.weight_g" not in sd
    c = {"generator_model": "parallel_wavegan_generator", "audio": {"num_mels": 80},
         "generator_model_params": {"upsample_factors": [4, 4, 4, 4], "stacks": 3, "num_res_blocks": 30}}
    v = setup_generator(c)
    assert isinstance(v, ParallelWaveganGenerator) and v.hop == 256
    with pytest.raises(NotImplementedError):
        ParallelWaveganGenerator(res_channels=32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.inference(torch.zeros(1, 80, 4))


def test_bidirectional_decoder_keys():
    """bidirectional_decoder=True: decoder_backward.* mirrors decoder.* (tacotron_abstract.py:104-105),
    registered before coarse_decoder (checked against the reference module when it was built)."""
    m = Tacotron2(num_chars=129, r=7, double_decoder_consistency=True, ddc_r=7, bidirectional_decoder=True)
    keys = list(m.state_dict().keys())
    dec = [k for k in keys if k.startswith("decoder.")]
    bwd = [k for k in keys if k.startswith("decoder_backward.")]
    assert bwd == ["decoder_backward." + k[len("decoder."):] for k in dec]
    assert keys.index(bwd[-1]) < keys.index("coarse_decoder.prenet.linear_layers.0.linear_layer.weight")


class _FakeTacoEngine:
    """Stands in for the library context: records the chunks the host logic hands it and fills
    each row's outputs with recognisable values up to that row's own step count."""

    def __init__(self):
        import threading
        self.lock = threading.RLock()
        self.weight_keys = {}
        self.calls = []
        self.max_steps_rows = None  # rows per call that report status 2 (None: all of them)

    def load_tacotron(self, *a, **k):
        pass

    load_tacotron1 = load_tacotron

    def taco_infer(self, ids, lens, r, ms, S_cap, thr, dec, post, align, stop, speaker_ids=None,
                   speaker_embeddings=None):
        assert self.lock._is_owned()  # the model holds the engine lock across the call
        nb = ids.shape[0]
        self.calls.append((nb, S_cap, ids.shape[1]))
        steps = np.asarray(ms, np.int32).copy()
        dec.zero_(), post.zero_(), align.zero_(), stop.zero_()
        for i in range(nb):
            tag = float(ids[i, 0])
            dec[i, :steps[i] * r] = tag
            post[i, :steps[i] * r] = tag + 0.5
            align[i, :steps[i], :int(lens[i])] = tag
            stop[i, :steps[i]] = tag
        k = nb if self.max_steps_rows is None else self.max_steps_rows
        return steps, np.where(np.arange(nb) < k, 2, 1).astype(np.int32)

    def tacotron1_infer(self, ids, lens, r, ms, S_cap, dec, post, align, stop):
        return self.taco_infer(ids, lens, r, ms, S_cap, None, dec, post, align, stop)


def _fake_engine(monkeypatch):
    """Every model finds its engine through tts_amd._lib.get_engine, looked up at call time."""
    eng = _FakeTacoEngine()
    monkeypatch.setattr("tts_amd._lib.get_engine", lambda dev: eng)
    return eng


def _ragged_batch(rs, B, long_row):
    """B padded rows tagged i + 1 with random lengths and step counts; ``long_row`` decodes longest."""
    lens = rs.randint(1, 30, B)
    steps = rs.randint(1, 6, B)
    steps[long_row] = 17
    ids = np.zeros((B, lens.max()), np.int64)
    for i in range(B):
        ids[i, :lens[i]] = i + 1
    return ids, lens, steps


def _check_joined_rows(outs, lens, steps, r):
    dec, post, align, stop = outs
    for i in range(len(lens)):
        M = r * steps[i]
        assert (dec[i, :M] == i + 1).all() and not dec[i, M:].any()
        assert (post[i, :M] == i + 1.5).all() and not post[i, M:].any()
        assert (align[i, :steps[i], :lens[i]] == i + 1).all() and not align[i, :, lens[i]:].any()
        assert not align[i, steps[i]:].any() and not stop[i, steps[i]:].any()


def test_tacotron2_multichunk_join_ragged_steps(monkeypatch):
    """B = 70 splits into chunks of 64 and 6 that decode to different S_cap (the second chunk
    longer than the first, then shorter): every row keeps its own frames and zero padding, in
    the caller's order (the join used to assume equal chunk lengths)."""
    eng = _fake_engine(monkeypatch)
    m = Tacotron2(num_chars=129, r=7, attn_norm="sigmoid")
    m.decoder.set_r(2)
    m.decoder.verbose = False
    B = 70
    rs = np.random.RandomState(0)
    for long_chunk in (0, 1):
        ids, lens, steps = _ragged_batch(rs, B, 64 + 2 if long_chunk else 5)  # the longest row sits in one chunk only
        eng.calls.clear()
        dec, post, align, stop = m.inference(torch.from_numpy(ids), text_lengths=lens, max_decoder_steps=steps)
        assert [c[0] for c in eng.calls] == [64, 6]
        S = int(steps.max())
        assert dec.shape == (B, 2 * S, 80) and post.shape == (B, 2 * S, 80)
        assert align.shape == (B, S, lens.max()) and stop.shape == (B, S, 1)
        _check_joined_rows((dec, post, align, stop), lens, steps, 2)
        assert list(m.last_steps) == list(steps)


def test_tacotron1_multichunk_join_ragged_steps(monkeypatch):
    """The same 64 + 6 split through Tacotron (v1): each library call gets S_cap = its rows' largest
    max_decoder_steps + 1, and the join keeps every row's own frames and zero padding."""
    from tts_amd import Tacotron
    eng = _fake_engine(monkeypatch)
    m = Tacotron(num_chars=129, num_speakers=0, r=5, postnet_output_dim=33)
    m.decoder.set_r(2)
    m.decoder.verbose = False
    B = 70
    rs = np.random.RandomState(0)
    for long_chunk in (0, 1):
        ids, lens, steps = _ragged_batch(rs, B, 64 + 2 if long_chunk else 5)
        eng.calls.clear()
        dec, post, align, stop = m.inference(torch.from_numpy(ids), text_lengths=lens, max_decoder_steps=steps)
        assert eng.calls == [(64, int(steps[:64].max()) + 1, int(lens[:64].max())),
                             (6, int(steps[64:].max()) + 1, int(lens[64:].max()))]
        S = int(steps.max())
        assert dec.shape == (B, 2 * S, 80) and post.shape == (B, 2 * S, 33)
        assert align.shape == (B, S, lens.max()) and stop.shape == (B, S, 1)
        _check_joined_rows((dec, post, align, stop), lens, steps, 2)
        assert list(m.last_steps) == list(steps) and list(m.last_mel_lengths) == list(2 * steps)


@pytest.mark.parametrize("v1", [False, True])
def test_decoder_stop_line_is_printed_once_per_row_at_max_steps(monkeypatch, capsys, v1):
    """layers/tacotron2.py:365, layers/tacotron.py:493: one line per row that ran into
    max_decoder_steps, unless ``decoder.verbose`` is False."""
    from tts_amd import Tacotron
    eng = _fake_engine(monkeypatch)
    m = Tacotron(num_chars=129, num_speakers=0, postnet_output_dim=33) if v1 else Tacotron2(num_chars=129, r=2)
    ids = torch.ones(5, 4, dtype=torch.long)
    eng.max_steps_rows = 3
    m.inference(ids, max_decoder_steps=2)
    assert capsys.readouterr().out == "   | > Decoder stopped with 'max_decoder_steps\n" * 3
    assert list(m.last_status) == [2, 2, 2, 1, 1]
    m.decoder.verbose = False
    m.inference(ids, max_decoder_steps=2)
    assert capsys.readouterr().out == ""


def test_single_speaker_model_ignores_speaker_arguments(monkeypatch):
    """models/tacotron2.py:152: speaker_ids / speaker_embeddings are ignored when num_speakers <= 1."""
    _fake_engine(monkeypatch)
    m = Tacotron2(num_chars=129, r=2, attn_norm="sigmoid")
    m.decoder.verbose = False
    ids = torch.ones(1, 5, dtype=torch.long)
    a = m.inference(ids, max_decoder_steps=3)
    b = m.inference(ids, speaker_ids=torch.tensor([3]), speaker_embeddings=torch.ones(1, 256),
                    max_decoder_steps=3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


class _RecordingEngine:
    """Records every ``load_*`` call as (method, tensor names, finalize arguments)."""

    def __init__(self):
        self.weight_keys = {}
        self.loads = []
        self.fail = False

    def __getattr__(self, name):
        if not name.startswith("load_"):
            raise AttributeError(name)

        def load(tensors, *args):
            if self.fail:  # as the library: the old weights are gone by the time finalize throws
                raise RuntimeError("ttship: model not finalized")
            self.loads.append((name, list(tensors), args))
        return load


def _sync_cases():
    from tts_amd import (FullbandMelganGenerator, GlowTts, MelganGenerator, ParallelWaveganGenerator, SpeakerEncoder,
                         Tacotron)
    taco = ("coarse_decoder.", "decoder_backward.")
    pqmf = ("pqmf_layer.H", "pqmf_layer.updown")
    # name: (constructor, slot, load method, skipped state_dict prefixes, finalize arguments)
    return {
        "tacotron2": (lambda: Tacotron2(num_chars=129, r=7, attn_norm="sigmoid", double_decoder_consistency=True,
                                        ddc_r=7), "taco", "load_tacotron", taco,
                      (129, 7, "sigmoid", False, False, False)),
        "tacotron": (lambda: Tacotron(num_chars=129, num_speakers=0), "tacotron1", "load_tacotron1", taco,
                     (129, 5, 5, "sigmoid", 1025)),
        "melgan": (MelganGenerator, "melgan", "load_melgan", pqmf, (80, 1, 512, (8, 8, 2, 2), 3, False)),
        "multiband_melgan": (lambda: MultibandMelganGenerator(upsample_factors=(8, 4, 2), num_res_blocks=4),
                             "melgan", "load_melgan", pqmf, (80, 4, 384, (8, 4, 2), 4, True)),
        "fullband_melgan": (FullbandMelganGenerator, "melgan", "load_melgan", pqmf,
                            (80, 1, 512, (2, 8, 2, 2), 4, False)),
        "pwgan": (ParallelWaveganGenerator, "pwgan", "load_pwgan", (), (30, 3, (4, 4, 4, 4))),
        "ge2e": (lambda: SpeakerEncoder(input_dim=40), "ge2e", "load_ge2e", (), (40, 256, 768, 3, True)),
        "glow": (lambda: GlowTts(num_chars=130), "glow", "load_glow", (), (130, 9, 12, 4)),
    }


SYNC_CASES = ["tacotron2", "tacotron", "melgan", "multiband_melgan", "fullband_melgan", "pwgan", "ge2e", "glow"]


@pytest.mark.parametrize("case", SYNC_CASES)
def test_sync_loads_once_per_weight_change(case):
    """``_sync`` uploads exactly when the engine's slot holds another model or another version of
    this one: what is uploaded (names, finalize arguments) and every event that bumps the version."""
    from tts_amd.params import host_tensors
    make, slot, method, skip, final = _sync_cases()[case]
    eng, m = _RecordingEngine(), make()
    m._sync(eng)
    assert len(eng.loads) == 1
    name, names, args = eng.loads[0]
    assert name == method and args == final
    assert names == list(host_tensors(m, skip_prefixes=skip))
    assert not any(n.startswith(p) for n in names for p in skip)
    if case == "tacotron2":
        assert any(k.startswith("coarse_decoder.") for k in m.state_dict())
    if case == "multiband_melgan":
        assert "pqmf_layer.H" in m.state_dict() and "pqmf_layer.G" in names
    m._sync(eng)
    assert len(eng.loads) == 1
    bumps = [m.invalidate, lambda: m.load_state_dict(m.state_dict()), m.float]
    if hasattr(m, "remove_weight_norm"):
        bumps.append(m.remove_weight_norm)
    for n, bump in enumerate(bumps, 2):
        bump()
        m._sync(eng)
        assert len(eng.loads) == n
        m._sync(eng)
        assert len(eng.loads) == n
    if hasattr(m, "remove_weight_norm"):
        assert not any(k.endswith(("weight_g", "weight_v")) for k in eng.loads[-1][1])
    other = make()
    for n, model in enumerate((other, m, other, m), len(eng.loads) + 1):
        model._sync(eng)
        assert len(eng.loads) == n
    assert eng.weight_keys == {slot: m.weight_key}


def test_melgan_family_shares_one_slot():
    from tts_amd import FullbandMelganGenerator, MelganGenerator
    eng = _RecordingEngine()
    models = [MelganGenerator(), MultibandMelganGenerator(upsample_factors=(8, 4, 2), num_res_blocks=4),
              FullbandMelganGenerator()]
    for n, m in enumerate(models + models, 1):
        m._sync(eng)
        assert len(eng.loads) == n and eng.weight_keys == {"melgan": m.weight_key}


@pytest.mark.parametrize("case", SYNC_CASES)
def test_failed_load_empties_the_slot(case):
    """The library drops a slot's weights before a load can fail, so the model that held the slot
    must upload again afterwards instead of finding its old key there."""
    make, slot = _sync_cases()[case][:2]
    eng, a, b = _RecordingEngine(), make(), make()
    a._sync(eng)
    eng.fail = True
    with pytest.raises(RuntimeError, match="not finalized"):
        b._sync(eng)
    assert eng.weight_keys[slot] is None
    eng.fail = False
    a._sync(eng)
    assert len(eng.loads) == 2 and eng.weight_keys[slot] == a.weight_key


@pytest.mark.parametrize("case", SYNC_CASES)
def test_reload_counter_stays_out_of_saved_checkpoints(case):
    """state_dict()._metadata carries nn.Module._version, torch's format version of the module; the
    models' reload counter must not shadow it."""
    m = _sync_cases()[case][0]()
    before = m.weight_key
    m.invalidate()
    m.invalidate()
    assert m.weight_key == (before[0], before[1] + 2)
    assert m.state_dict()._metadata[""]["version"] == torch.nn.Module._version
    assert "_version" not in vars(m)


def test_runtime_switch_table_matches_switches_header():
    """tts_amd/csrc/switches.h is the one place the library reads its environment: the TTS_* names in
    its string literals are exactly the rows of INTEGRATION.md's "Run-time switches" table, and no
    other file under tts_amd/csrc/ calls getenv."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "tts_amd", "csrc")
    header = open(os.path.join(csrc, "switches.h")).read()
    in_header = set()
    for lit in re.findall(r'"((?:[^"\\\n]|\\.)*)"', header):
        in_header.update(re.findall(r"TTS_[A-Z0-9_]+", lit))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    section = doc.split("### Run-time switches", 1)[1].split("\n## ", 1)[0]
    in_table = set()
    for row in section.splitlines():
        if row.startswith("| `"):  # the name is the first cell
            in_table.update(re.findall(r"TTS_[A-Z0-9_]+", row.split("|")[1]))
    assert in_header and in_header == in_table, (sorted(in_header - in_table), sorted(in_table - in_header))
    others = [f for f in sorted(os.listdir(csrc))
              if f != "switches.h" and os.path.isfile(os.path.join(csrc, f))
              and "getenv" in open(os.path.join(csrc, f), errors="ignore").read()]
    assert others == [], others


# every synchronous or one-off host-to-device copy the library may make: (file, text of the line) -> why
_H2D_ALLOWED = {
    ("host.h", "HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));"):
        "DevBuf::upload: synchronous weight and table uploads at load time",
    ("api_core.hip", "HIP_OK(hipMemcpy(L.W16.p, w16.data(), w16.size() * 2, hipMemcpyHostToDevice));"):
        "pack_conv / pack_conv_x3_only: the split-f16 weights, synchronous, at load time",
    ("api_taco.hip", "HIP_OK(hipMemcpyAsync(W.fwd_u.p, half.data(), 64 * 4, hipMemcpyHostToDevice, s));"):
        "forward attention's initial u = 0.5: the source is a static const array",
    ("api_taco_graph.hip", "HIP_OK(hipMemcpyAsync(W.ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice, s));"):
        "tts_time_decoder_kernel: the timing entry re-arms the control block, and synchronises before it returns",
    ("api_taco_graph.hip", "HIP_OK(hipMemcpy(W.ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice));"):
        "tts_time_decoder_kernel: synchronous restore of the control block",
}


def test_host_to_device_copies_are_allow_listed():
    """Per-call row arrays (lengths, ids) reach the device as kernel arguments (put_rows, RowInts), never
    through a copy from a host buffer that may die or stall the stream: every line of the library that
    names hipMemcpyHostToDevice is one of the listed load-time or static-source copies."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tts_amd", "csrc")
    seen = set()
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h")):
            continue
        for no, line in enumerate(open(os.path.join(csrc, name)), 1):
            if "hipMemcpyHostToDevice" in line:
                key = (name, line.strip())
                assert key in _H2D_ALLOWED, f"{name}:{no}: host-to-device copy outside the allow-list: {line.strip()}"
                seen.add(key)
    assert seen == set(_H2D_ALLOWED), f"allow-list entries that match nothing: {set(_H2D_ALLOWED) - seen}"
    assert all(reason for reason in _H2D_ALLOWED.values())
