"""Generate the teacher-forcing fixtures by running the REFERENCE ``Tacotron2.forward`` on the CPU.

Run where the reference checkout is (``TTS_REFERENCE``, as for make_golden.py), from the repository
root; no GPU is needed:

    python tests/golden/make_teacher_golden.py [taco_teacher] [taco_teacher_bnspk]

``forward(text, text_lengths, mel_specs, mel_lengths)`` in ``eval()`` is the call of
``notebooks/ExtractTTSpectrogram.ipynb``: a decode driven by the ground-truth mel. Every row is
run alone (B = 1) on its own ``S * r`` frames, ``S = ceil(M / r)``, which is what a batched call of
this package returns per row. Teacher mels are the same model's free-running postnet output for
the row, cut or zero-extended to M frames, plus ``0.25 sin(0.37 n + 0.11 c)``. Only seeds and
gains are stored, never weights.

    taco_teacher.npz        the taco_sigmoid fixture's weights, r in {2, 1},
                            rows (T, M) = (12, 140), (37, 9), (80, 10), (5, 1)
    taco_teacher_bnspk.npz  softmax norm + BN prenet, r = 2, two rows: learned speaker table
                            (``tab_*``) and external 256-d speaker embeddings (``ext_*``)
"""

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import STOP_GAIN, build_taco, run_taco  # noqa: E402
from tts_amd.spec import TacotronConfig  # noqa: E402

MEL_TOL = 1e-4
ROWS = ((12, 140), (37, 9), (80, 10), (5, 1))  # (T, M); T = 12, 37, 80 are taco_sigmoid's utterances


def teacher_mel(free_post, M):
    """The row's free-running postnet output cut or zero-extended to M frames, plus a sinusoid."""
    mel = np.zeros((M, 80), np.float64)
    n = min(M, len(free_post))
    mel[:n] = free_post[:n]
    nn, cc = np.meshgrid(np.arange(M), np.arange(80), indexing="ij")
    return (mel + 0.25 * np.sin(0.37 * nn + 0.11 * cc)).astype(np.float32)


def run_forward(m, ids, mel, r, dtype=torch.float32, spk=None):
    """Reference forward on one row: (dec (S r, 80), post (S r, 80), align (S, T), stop logits (S))."""
    M = len(mel)
    S = -(-M // r)
    padded = np.zeros((1, S * r, 80), np.float32)
    padded[0, :M] = mel
    m.decoder.set_r(r)
    kw = {}
    if spk is not None and np.ndim(spk) == 0:
        kw["speaker_ids"] = torch.tensor([int(spk)])
    elif spk is not None:
        kw["speaker_embeddings"] = torch.from_numpy(np.asarray(spk)[None]).to(dtype)
    torch.set_default_dtype(dtype)
    with torch.no_grad():
        out = m.forward(torch.from_numpy(ids[None].astype(np.int64)), torch.tensor([len(ids)]),
                        torch.from_numpy(padded).to(dtype), torch.tensor([M]), **kw)
    torch.set_default_dtype(torch.float32)
    dec, post, align, stop = (o[0].double().numpy() for o in out[:4])  # DDC models add two training tensors
    assert dec.shape == (S * r, 80) and post.shape == (S * r, 80) and align.shape == (S, len(ids)) and stop.shape == (S,)
    return dec, post, align, stop


def teacher_row(out, key, m32, m64, ids, r, M, max_steps, spk=None, m_free=None):
    """One fixture row under ``key``; returns (drift64, stop_drift64). ``m_free``: the model of the
    free-running decode where its stop bias differs (the bias never changes the frames)."""
    free = run_taco(m_free or m32, ids, r, max_steps, spk=spk)
    free_dec, free_post = free[0], free[1]
    mel = teacher_mel(free_post, M)
    dec, post, align, stop = run_forward(m32, ids, mel, r, spk=spk)
    dec64, post64, _, stop64 = run_forward(m64, ids, mel, r, torch.float64, spk=spk)
    drift = float(max(np.abs(dec - dec64).max(), np.abs(post - post64).max()))
    sdrift = float(np.abs(stop - stop64).max())
    assert 8 * drift <= MEL_TOL, (key, drift)
    # frames past M are exactly zero in the reference's masked outputs
    assert not dec[M:].any() and not post[M:].any(), key
    if M >= 2:  # the teacher-forced frames are not the free-running ones
        n = min(M, len(free_dec))
        diff = float(np.abs(dec[:n] - free_dec[:n]).max())
        assert diff >= 50 * MEL_TOL, (key, diff)
    else:
        diff = 0.0
    out[key + "_ids"] = ids
    out[key + "_mel"] = mel
    out[key + "_M"] = np.int64(M)
    out[key + "_dec"] = dec.astype(np.float32)
    out[key + "_post"] = post.astype(np.float32)
    out[key + "_align"] = align.astype(np.float32)
    out[key + "_stop_logit"] = stop.astype(np.float32)
    out[key + "_drift64"] = np.float64(drift)
    out[key + "_stop_drift64"] = np.float64(sdrift)
    if spk is not None:
        out[key + "_spk"] = np.asarray(spk, np.float32 if np.ndim(spk) else np.int64)
    print(f"  {key} T={len(ids)} M={M} drift64={drift:.2e} stop_drift64={sdrift:.2e} vs free-running {diff:.2e}")
    return drift, sdrift


def finish(name, out, sdrifts):
    stop_tol = 64 * max(sdrifts)
    assert stop_tol <= 1e-3, stop_tol
    out["stop_tol"] = np.float64(stop_tol)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"[{name}] stop_tol {stop_tol:.2e}, {os.path.getsize(os.path.join(HERE, name + '.npz')) / 1024:.0f} KiB")


def teacher_case(name="taco_teacher"):
    src = np.load(os.path.join(HERE, "taco_sigmoid.npz"))
    cfg = TacotronConfig(**json.loads(str(src["cfg"])))
    gains = json.loads(str(src["overrides"]))
    out = {"cfg": str(src["cfg"]), "overrides": str(src["overrides"]), "seed": src["seed"], "r_list": np.array([2, 1])}
    short = np.random.RandomState(71).randint(1, cfg.num_chars, size=5).astype(np.int64)
    sdrifts = []
    for r in (2, 1):
        seed = int(src[f"r{r}_seed"]) if f"r{r}_seed" in src.files else int(src["seed"])
        bias = float(src[f"r{r}_stop_bias"])
        out[f"r{r}_seed"] = np.int64(seed)
        out[f"r{r}_stop_bias"] = np.float32(bias)
        m32 = build_taco(cfg, seed, bias, gains=gains)
        m64 = build_taco(cfg, seed, bias, torch.float64, gains=gains)
        print(f"[{name}] r={r}")
        for i, (T, M) in enumerate(ROWS):
            ids = src[f"r{r}_u{i}_ids"] if i < 3 else short
            assert len(ids) == T
            sdrifts.append(teacher_row(out, f"r{r}_u{i}", m32, m64, ids, r, M, int(src[f"r{r}_max_steps"]))[1])
    finish(name, out, sdrifts)


def bnspk_case(name="taco_teacher_bnspk"):
    """Softmax norm, BN prenet, r = 2. Stop bias 0 (at the -1e4 that keeps the free-running decode
    from stopping, the logits' fp32 spacing alone is 1e-3); the free-running decode runs 30 steps."""
    out = {"overrides": json.dumps(STOP_GAIN), "stop_bias": np.float32(0.0), "r": np.int64(2)}
    rows = ((21, 37), (33, 24))  # M = 37: a padded last group
    rs = np.random.RandomState(75)
    utts = [rs.randint(1, 129, size=T).astype(np.int64) for T, _ in rows]
    embs = [(rs.randn(256) / 16.0).astype(np.float32) for _ in rows]
    embs = [e / np.linalg.norm(e) for e in embs]
    sdrifts = []
    for tag, seed, cfg, spks in (
            ("tab", 73, TacotronConfig(attn_norm="softmax", prenet_type="bn", num_speakers=4), [3, 1]),
            ("ext", 74, TacotronConfig(attn_norm="softmax", prenet_type="bn", num_speakers=4,
                                       speaker_embedding_dim=256), embs)):
        out[tag + "_cfg"] = json.dumps(cfg.__dict__)
        out[tag + "_seed"] = np.int64(seed)
        m_free = build_taco(cfg, seed, -1e4)
        m32 = build_taco(cfg, seed, 0.0)
        m64 = build_taco(cfg, seed, 0.0, torch.float64)
        print(f"[{name}] {tag}")
        for i, (T, M) in enumerate(rows):
            sdrifts.append(teacher_row(out, f"{tag}_u{i}", m32, m64, utts[i], 2, M, 30, spk=spks[i], m_free=m_free)[1])
    finish(name, out, sdrifts)


if __name__ == "__main__":
    which = sys.argv[1:] or ["taco_teacher", "taco_teacher_bnspk"]
    if "taco_teacher" in which:
        teacher_case()
    if "taco_teacher_bnspk" in which:
        bnspk_case()
