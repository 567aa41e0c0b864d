"""GPU parity of Global Style Tokens on multi-speaker Tacotron2 against the reference (fixtures:
tests/golden/make_gst_golden.py; ``ext`` = external 256-d speaker embeddings that also enter the style
query, G 512 / 4 heads / 10 tokens; ``tab`` = learned speaker table, G 256 / 8 heads / 5 tokens, BN prenet).

Tolerances: style vectors <= the fixture's ``style_tol`` (8 x the reference's own fp32-vs-fp64 drift on
these inputs, 3.0e-6 / 3.7e-6 at magnitude 1.8 / 1.3); frames <= MEL_TOL (1e-4, at least 8 x the
reference's drift, asserted by the generator); alignments <= 1e-5 with exact argmax above the 1e-5
margin and exact stop steps, as in test_gpu_parity; forward's stop logits <= ``stop_tol``. Rows of a
batch are compared bit for bit with their own B = 1 call."""
import json

import numpy as np
import pytest
import torch

from gst_helpers import build_gst_taco, gst_fixture, gst_state_dict
from helpers import build_melgan, melgan_state_dict

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4
ALIGN_MARGIN = 1e-5
TAGS = ["ext", "tab"]


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


_models = {}


def _model(tag):
    if tag not in _models:
        fx, cfg = gst_fixture(tag)
        m = build_gst_taco(cfg, gst_state_dict(fx, cfg), _dev())
        m.decoder.set_r(int(fx["r"]))
        m.decoder.max_decoder_steps = int(fx["max_steps"])
        m.decoder.verbose = False
        _models[tag] = (fx, cfg, m)
    return _models[tag]


def _ext(cfg):
    return cfg.speaker_embedding_dim is not None


def _spk_kw(fx, cfg, rows):
    """The speaker argument of fixture speakers ``rows`` (indices into style_spk)."""
    spk = torch.from_numpy(fx["style_spk"][list(rows)]).to(_dev())
    return {"speaker_embeddings" if _ext(cfg) else "speaker_ids": spk}


def _style(m, cfg, fx, mel, rows, lengths=None):
    emb = torch.from_numpy(fx["style_spk"][list(rows)]) if cfg.gst_query_speaker_dim else None
    return m.style_embedding(mel, style_lengths=lengths, speaker_embeddings=emb)


@pytest.mark.parametrize("tag", TAGS)
def test_style_embeddings_match_the_reference(tag):
    fx, cfg, m = _model(tag)
    for i, N in enumerate(fx["style_n"]):
        out = _style(m, cfg, fx, torch.from_numpy(fx[f"style_mel_{N}"][None]), [i])
        assert out.shape == (1, cfg.gst_embedding_dim)
        err = np.abs(out[0].cpu().numpy() - fx[f"style_{N}"]).max()
        print(f"gst-style-err {tag} N={N}: {err:.2e} (tol {float(fx['style_tol']):.2e})")
        assert err <= float(fx["style_tol"]), (N, err)


@pytest.mark.parametrize("tag", TAGS)
def test_padded_unsorted_batch_is_bit_identical_to_single_rows(tag):
    """All five lengths in one batch, neither sorted nor grouped, padding filled with 1e3: no row may
    read past its own frames, and a row's sums do not depend on its batch."""
    fx, cfg, m = _model(tag)
    order = [1, 4, 0, 3, 2]  # N = 37, 130, 1, 65, 64
    Ns = [int(fx["style_n"][i]) for i in order]
    mel = np.full((len(order), max(Ns), 80), 1e3, np.float32)
    for b, (i, N) in enumerate(zip(order, Ns)):
        mel[b, :N] = fx[f"style_mel_{N}"]
    out = _style(m, cfg, fx, torch.from_numpy(mel), order, lengths=Ns)
    for b, (i, N) in enumerate(zip(order, Ns)):
        one = _style(m, cfg, fx, torch.from_numpy(fx[f"style_mel_{N}"][None]), [i])
        assert torch.equal(out[b], one[0]), N
        assert np.abs(out[b].cpu().numpy() - fx[f"style_{N}"]).max() <= float(fx["style_tol"])


@pytest.mark.parametrize("tag", TAGS)
def test_untransposed_mel_is_read_as_rows_of_80(tag):
    """synthesis() hands over (1, 80, N): the model reads that memory as (1, N, 80), as the reference's view does."""
    fx, cfg, m = _model(tag)
    x = torch.from_numpy(np.ascontiguousarray(fx["style_mel_65"].T)[None])  # (1, 80, 65)
    a = _style(m, cfg, fx, x, [3])
    b = _style(m, cfg, fx, x.reshape(1, -1, 80), [3])
    assert torch.equal(a, b)
    c = _style(m, cfg, fx, torch.from_numpy(fx["style_mel_65"][None]), [3])
    assert (a - c).abs().max() > 1000 * float(fx["style_tol"])  # and not as its transpose


@pytest.mark.parametrize("tag", TAGS)
def test_token_dict_style(tag):
    fx, cfg, m = _model(tag)
    out = m.style_embedding(json.loads(str(fx["style_dict"])))
    err = np.abs(out[0].cpu().numpy() - fx["dict_style"]).max()
    print(f"gst-dict-err {tag}: {err:.2e}")
    assert err <= float(fx["style_tol"])
    assert not m.style_embedding(None).any()


def _check_infer(fx, key, b, dec, post, align, stop, steps, r):
    S = len(fx[key + "_stop"])
    assert steps[b] == S, f"{key}: steps {steps[b]} != reference {S}"
    M = S * r
    errs = (np.abs(dec[b, :M] - fx[key + "_dec"]).max(), np.abs(post[b, :M] - fx[key + "_post"]).max())
    print(f"gst-infer-err {key} row {b}: dec {errs[0]:.2e} post {errs[1]:.2e}")
    assert errs[0] <= MEL_TOL and errs[1] <= MEL_TOL, (key, errs)
    assert not post[b, M:].any() and not dec[b, M:].any()
    T = fx[key + "_align"].shape[1]
    a = align[b, :S, :T]
    assert np.abs(a - fx[key + "_align"]).max() <= 1e-5
    sel = fx[key + "_top2"] > ALIGN_MARGIN
    assert np.array_equal(a.argmax(1)[sel], fx[key + "_align"].argmax(1)[sel])
    assert np.abs(stop[b, :S, 0] - fx[key + "_stop"]).max() <= 1e-4
    assert not align[b, S:].any() and not align[b, :, T:].any()


def _infer(m, fx, cfg, keys, spk_rows, style, style_lengths=None):
    dev = _dev()
    ids = [fx[k + "_ids"] for k in keys]
    text = np.zeros((len(keys), max(len(i) for i in ids)), np.int64)
    for b, i in enumerate(ids):
        text[b, :len(i)] = i
    out = m.inference(torch.from_numpy(text).to(dev), style_mel=style, style_lengths=style_lengths,
                      text_lengths=[len(i) for i in ids], **_spk_kw(fx, cfg, spk_rows))
    return [o.cpu().numpy() for o in out] + [m.last_steps]


@pytest.mark.parametrize("tag", TAGS)
def test_inference_each_row_alone(tag):
    """Three texts with a style mel each, one with the token dict, one with style_mel=None (the
    fixture's zero-style run)."""
    fx, cfg, m = _model(tag)
    r = int(fx["r"])
    for u in range(3):
        mel = torch.from_numpy(fx[f"style_mel_{int(fx['infer_style_n'][u])}"][None])
        out = _infer(m, fx, cfg, [f"u{u}"], [u], mel)
        _check_infer(fx, f"u{u}", 0, *out, r)
    out = _infer(m, fx, cfg, ["d0"], [0], json.loads(str(fx["style_dict"])))
    _check_infer(fx, "d0", 0, *out, r)
    out = _infer(m, fx, cfg, ["z1"], [1], None)
    _check_infer(fx, "z1", 0, *out, r)


def _style_batch(fx, us):
    """Style mels of the texts ``us`` as one batch padded with 1e3, and their lengths."""
    Ns = [int(fx["infer_style_n"][u]) for u in us]
    mel = np.full((len(us), max(Ns), 80), 1e3, np.float32)
    for b, N in enumerate(Ns):
        mel[b, :N] = fx[f"style_mel_{N}"]
    return torch.from_numpy(mel), Ns


@pytest.mark.parametrize("tag", TAGS)
def test_inference_unsorted_batch(tag):
    """Caller order (T, style N) = (9, 65), (40, 130), (23, 37): sorted in neither, so the style rows
    go through the decode-order permutation with the speaker rows."""
    fx, cfg, m = _model(tag)
    us = [2, 1, 0]
    mel, Ns = _style_batch(fx, us)
    out = _infer(m, fx, cfg, [f"u{u}" for u in us], us, mel, Ns)
    for b, u in enumerate(us):
        _check_infer(fx, f"u{u}", b, *out, int(fx["r"]))


def test_seventeen_rows_cross_the_batch_tile():
    fx, cfg, m = _model("ext")
    us = [0, 1, 2] * 5 + [1, 0]
    mel, Ns = _style_batch(fx, us)
    out = _infer(m, fx, cfg, [f"u{u}" for u in us], us, mel, Ns)
    for b, u in enumerate(us):
        _check_infer(fx, f"u{u}", b, *out, int(fx["r"]))


def _check_forward_row(out, b, fx, key, r):
    dec, post, align, stop = out
    M, T = int(fx[key + "_M"]), len(fx[key + "_ids"])
    S = -(-M // r)
    errs = (np.abs(dec[b, :S * r] - fx[key + "_dec"]).max(), np.abs(post[b, :S * r] - fx[key + "_post"]).max(),
            np.abs(align[b, :S, :T] - fx[key + "_align"]).max(), np.abs(stop[b, :S] - fx[key + "_stop_logit"]).max())
    print(f"gst-forward-err {key} row {b}: dec {errs[0]:.2e} post {errs[1]:.2e} align {errs[2]:.2e} stop {errs[3]:.2e}")
    assert errs[0] <= MEL_TOL and errs[1] <= MEL_TOL and errs[2] <= MEL_TOL, (key, errs)
    assert errs[3] <= float(fx["stop_tol"]), (key, errs)
    assert not dec[b, M:].any() and not post[b, M:].any(), key
    assert not align[b, S:].any() and not align[b, :, T:].any() and not stop[b, S:].any(), key


@pytest.mark.parametrize("tag", TAGS)
def test_forward_takes_each_rows_style_from_its_own_teacher_mel(tag):
    """Rows (T, M) = (23, 24), (9, 37) as one batch (teacher padding 1e3; M = 37 has a padded last
    group, whose zero frame is part of the row's style input), then the second row alone."""
    fx, cfg, m = _model(tag)
    r, dev = int(fx["r"]), _dev()
    for keys in (["f0", "f1"], ["f1"]):
        ids = [fx[k + "_ids"] for k in keys]
        mels = [fx[k + "_mel"] for k in keys]
        T, M = max(len(i) for i in ids), max(-(-len(x) // r) * r for x in mels)
        text = np.zeros((len(keys), T), np.int64)
        mel = np.full((len(keys), M, 80), 1e3, np.float32)
        for b, (i, x) in enumerate(zip(ids, mels)):
            text[b, :len(i)] = i
            mel[b, :len(x)] = x
        spk = torch.from_numpy(np.stack([fx[k + "_spk"] for k in keys])).to(dev)
        out = m.forward(torch.from_numpy(text).to(dev), torch.tensor([len(i) for i in ids]),
                        torch.from_numpy(mel).to(dev), torch.tensor([len(x) for x in mels]),
                        **{"speaker_embeddings" if _ext(cfg) else "speaker_ids": spk})
        out = [o.cpu().numpy() for o in out]
        for b, k in enumerate(keys):
            _check_forward_row(out, b, fx, k, r)


def test_inference_vocoded_with_a_style_is_the_two_calls():
    fx, cfg, m = _model("ext")
    dev = _dev()
    vcfg, vsd = melgan_state_dict(5)
    voc = build_melgan(vcfg, vsd, dev)
    ids = torch.from_numpy(fx["u2_ids"][None]).to(dev)
    mel = torch.from_numpy(fx["style_mel_65"][None])
    kw = _spk_kw(fx, cfg, [2])
    dec, post, align, stop = m.inference(ids, style_mel=mel, **kw)
    wav = voc.inference(post.transpose(1, 2), lengths=m.last_mel_lengths)
    out = m.inference_vocoded(ids, voc, style_mel=mel, **kw)
    for a, b in zip(out, (dec, post, align, stop, wav)):
        assert torch.equal(a, b)
    assert len(fx["u2_stop"]) == post.shape[1] // int(fx["r"])
    sub = m.inference_vocoded_submit(ids, voc, style_mel=mel, **kw).result()
    assert torch.equal(sub[4], wav)
