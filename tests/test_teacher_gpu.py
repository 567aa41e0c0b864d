"""GPU parity of the teacher-forced ``Tacotron2.forward`` against the reference's own ``forward`` in
``eval()`` (fixtures: tests/golden/make_teacher_golden.py). Every row is compared with the
reference's B = 1 call on that row alone. Tolerances: frames and alignments <= MEL_TOL (1e-4, at
least 8 x the reference's own fp32-vs-fp64 drift, asserted by the generator), stop logits <= the
fixture's ``stop_tol`` (64 x their fp32-vs-fp64 drift), exact zeros past a row's own extent."""
import json

import numpy as np
import pytest
import torch

from helpers import build_taco, load_fixture, taco_state_dict
from tts_amd.spec import TacotronConfig

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


_models = {}


def _teacher(r):
    """(fixture, model at reduction factor r) on the taco_sigmoid weights; built once per r."""
    fx = load_fixture("taco_teacher")
    if r not in _models:
        cfg, sd = taco_state_dict(fx, r=r)
        m = build_taco(cfg, sd, _dev())
        m.decoder.set_r(r)
        m.decoder.verbose = False
        _models[r] = m
    return fx, _models[r]


def _spk_model(tag):
    fx = load_fixture("taco_teacher_bnspk")
    if tag not in _models:
        cfg = TacotronConfig(**json.loads(str(fx[tag + "_cfg"])))
        _, sd = taco_state_dict(None, seed=int(fx[tag + "_seed"]), overrides=json.loads(str(fx["overrides"])),
                                stop_bias=float(fx["stop_bias"]), cfg=cfg)
        m = build_taco(cfg, sd, _dev())
        m.decoder.set_r(int(fx["r"]))
        _models[tag] = m
    return fx, _models[tag]


def _forward(m, fx, keys, r, mel_lengths=True, **kw):
    """forward on the fixture rows ``keys`` as one padded batch; outputs as numpy. The padding of
    the teacher mel is filled with a large value: no row may read it."""
    dev = _dev()
    ids = [fx[k + "_ids"] for k in keys]
    mels = [fx[k + "_mel"] for k in keys]
    T = max(len(i) for i in ids)
    M = max(-(-len(x) // r) * r for x in mels)
    text = np.zeros((len(keys), T), np.int64)
    mel = np.full((len(keys), M, 80), 1e3, np.float32)
    for b, (i, x) in enumerate(zip(ids, mels)):
        text[b, :len(i)] = i
        mel[b, :len(x)] = x
    out = m.forward(torch.from_numpy(text).to(dev), torch.tensor([len(i) for i in ids]), torch.from_numpy(mel).to(dev),
                    torch.tensor([len(x) for x in mels]) if mel_lengths else None, **kw)
    assert len(out) == 4
    dec, post, align, stop = (o.cpu().numpy() for o in out)
    assert dec.shape == (len(keys), M, 80) and post.shape == dec.shape
    assert align.shape == (len(keys), M // r, T) and stop.shape == (len(keys), M // r)
    return dec, post, align, stop


def _check_row(out, b, fx, key, r):
    """Row b of a batch against fixture row ``key``: tolerances inside the row's extent, exact
    zeros outside it."""
    dec, post, align, stop = out
    M, T = int(fx[key + "_M"]), len(fx[key + "_ids"])
    S = -(-M // r)
    errs = (np.abs(dec[b, :S * r] - fx[key + "_dec"]).max(), np.abs(post[b, :S * r] - fx[key + "_post"]).max(),
            np.abs(align[b, :S, :T] - fx[key + "_align"]).max(), np.abs(stop[b, :S] - fx[key + "_stop_logit"]).max())
    print(f"teacher-err {key} row {b}: dec {errs[0]:.2e} post {errs[1]:.2e} align {errs[2]:.2e} stop {errs[3]:.2e}")
    assert errs[0] <= MEL_TOL and errs[1] <= MEL_TOL and errs[2] <= MEL_TOL, (key, errs)
    assert errs[3] <= float(fx["stop_tol"]), (key, errs)
    assert not dec[b, M:].any() and not post[b, M:].any(), key
    assert not align[b, S:].any() and not align[b, :, T:].any() and not stop[b, S:].any(), key


@pytest.mark.parametrize("u", [0, 1, 2, 3])
@pytest.mark.parametrize("r", [2, 1])
def test_each_row_alone_matches_the_reference_forward(r, u):
    fx, m = _teacher(r)
    key = f"r{r}_u{u}"
    out = _forward(m, fx, [key], r)
    _check_row(out, 0, fx, key, r)
    M = int(fx[key + "_M"])
    assert list(m.last_steps) == [-(-M // r)] and list(m.last_mel_lengths) == [M]


@pytest.mark.parametrize("r", [2, 1])
def test_unsorted_batch_matches_row_by_row(r):
    """Caller order (37, 9), (5, 1), (12, 140), (80, 10): sorted in neither T nor S, so the
    decode-order permutation and the teacher buffer's gather through it are exercised."""
    fx, m = _teacher(r)
    keys = [f"r{r}_u{u}" for u in (1, 3, 0, 2)]
    out = _forward(m, fx, keys, r)
    for b, k in enumerate(keys):
        _check_row(out, b, fx, k, r)


def test_seventeen_rows_cross_the_batch_tile():
    fx, m = _teacher(2)
    keys = [f"r2_u{u}" for u in [0, 1, 2, 3] * 4 + [1]]
    out = _forward(m, fx, keys, 2)
    for b, k in enumerate(keys):
        _check_row(out, b, fx, k, 2)


def test_one_teacher_frame_moves_the_next_step_only():
    """mel[0, r - 1] is step 1's prenet input: step 0 (the go frame) must not see it, step 1 must."""
    r = 2
    fx, m = _teacher(r)
    dev = _dev()
    ids = torch.from_numpy(fx["r2_u2_ids"][None]).to(dev)
    mel = torch.from_numpy(fx["r2_u2_mel"][None]).to(dev)
    a = m.forward(ids, [ids.shape[1]], mel)[0].cpu().numpy()
    mel2 = mel.clone()
    mel2[0, r - 1] += 0.5
    b = m.forward(ids, [ids.shape[1]], mel2)[0].cpu().numpy()
    assert np.array_equal(a[0, :r], b[0, :r])
    assert np.abs(a[0, r:2 * r] - b[0, r:2 * r]).max() > 10 * MEL_TOL


def test_mel_lengths_none_means_full_rows():
    fx, m = _teacher(2)
    out = _forward(m, fx, ["r2_u2"], 2, mel_lengths=False)  # M = 10 = 5 r: the whole mel
    _check_row(out, 0, fx, "r2_u2", 2)
    assert list(m.last_mel_lengths) == [10]


@pytest.mark.parametrize("tag", ["tab", "ext"])
def test_both_speaker_forms(tag):
    """Softmax norm + BN prenet + speakers: learned table (ids) and external embeddings, the two
    rows as one batch (different speakers) and the second alone."""
    fx, m = _spk_model(tag)
    keys = [f"{tag}_u0", f"{tag}_u1"]
    spk = np.stack([fx[k + "_spk"] for k in keys])
    arg = "speaker_ids" if tag == "tab" else "speaker_embeddings"
    out = _forward(m, fx, keys, 2, **{arg: torch.from_numpy(spk).to(_dev())})
    for b, k in enumerate(keys):
        _check_row(out, b, fx, k, 2)
    out = _forward(m, fx, keys[1:], 2, **{arg: torch.from_numpy(spk[1:]).to(_dev())})
    _check_row(out, 0, fx, keys[1], 2)


def test_inference_after_forward_is_unchanged():
    """Teacher mode leaves no state behind: the free-running decode still matches its fixture."""
    fx, m = _teacher(2)
    _forward(m, fx, ["r2_u1", "r2_u2"], 2)
    sig = load_fixture("taco_sigmoid")
    ids = torch.from_numpy(sig["r2_u0_ids"][None]).to(_dev())
    dec, post, align, stop = m.inference(ids, max_decoder_steps=int(sig["r2_max_steps"]))
    ref = sig["r2_u0_post"]
    assert post.shape[1] == len(ref)
    assert np.abs(post[0].cpu().numpy() - ref).max() <= MEL_TOL
    assert np.abs(stop[0, :, 0].cpu().numpy() - sig["r2_u0_stop"]).max() <= 1e-4  # sigmoids again, not logits


def test_sixty_five_rows_split_into_library_calls():
    """64 short rows and the 140-frame row last: two library calls with different step counts."""
    fx, m = _teacher(2)
    keys = [f"r2_u{1 + b % 3}" for b in range(64)] + ["r2_u0"]
    out = _forward(m, fx, keys, 2)
    assert m._last_call[2] == 2
    for b, k in enumerate(keys):
        _check_row(out, b, fx, k, 2)
