"""Generate the Global Style Token fixtures by running the REFERENCE multi-speaker ``Tacotron2`` with
``gst=True`` on the CPU.

Run where the reference checkout is (``TTS_REFERENCE``, as for make_golden.py), from the repository
root; no GPU is needed:

    python tests/golden/make_gst_golden.py [ext] [tab]

    taco_gst_ext.npz   external 256-d speaker embeddings, gst_use_speaker_embedding (the style
                       attention's query takes the embedding too), G = 512, 4 heads, 10 tokens,
                       sigmoid attention norm, r = 2, DDC coarse decoder present
    taco_gst_tab.npz   learned table of 4 speakers, G = 256, 8 heads, 5 tokens, softmax norm, BN prenet
    taco_gst_keys.json the reference's state_dict key / shape list of both models

Per fixture: the style embedding ``gst_layer(mel)`` of mels of N in STYLE_N frames, a token-weight
dict, ``inference`` of three texts with a style mel each (plus one with the dict and one with
``style_mel=None``), and eval ``forward`` of two rows (whose style input is the teacher mel itself).
Every run is repeated in float64; the drifts are stored, ``style_tol`` is 8 x the largest
style-embedding drift. Only seeds and gains are stored, never weights.

The inputs must make the reference itself pass what the GPU tests rely on, or this script fails:
8 x the mel drift fits under MEL_TOL, style embeddings of different mels differ by at least
1000 x style_tol, and a style moves the decoder output by at least 50 x MEL_TOL.
"""

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import STOP_GAIN, Tacotron2, choose_stop_bias  # noqa: E402
from make_teacher_golden import run_forward, teacher_mel  # noqa: E402
from tts_amd.spec import TacotronConfig, tacotron2_spec  # noqa: E402
from tts_amd.weights import synth_state_dict  # noqa: E402

MEL_TOL = 1e-4
STYLE_N = (1, 37, 64, 65, 130)  # one GRU step; odd widths at several conv layers; the 64 / 65 step boundary
# With the default initialisation the style embedding barely depends on the mel: larger style tokens
# (sharper token attention), GRU and attention weights make it move
GAINS = dict(STOP_GAIN, gst_tokens=3.0, gst_gru=2.5, gst_attn=3.0)
R, MAX_STEPS = 2, 30
TEXT_LENS = (23, 40, 9)
INFER_STYLE_N = (37, 130, 65)  # the style mel of each text

CASES = {
    "ext": TacotronConfig(attn_norm="sigmoid", r=R, num_speakers=4, speaker_embedding_dim=256, gst=True,
                          gst_embedding_dim=512, gst_num_heads=4, gst_style_tokens=10, gst_use_speaker_embedding=True),
    "tab": TacotronConfig(attn_norm="softmax", r=R, num_speakers=4, prenet_type="bn", double_decoder_consistency=False,
                          gst=True, gst_embedding_dim=256, gst_num_heads=8, gst_style_tokens=5),
}
SEEDS = {"ext": 91, "tab": 95}
STYLE_DICT = {"ext": {"0": 0.3, "7": -0.2, "3": 0.15}, "tab": {"4": 0.25, "1": -0.1}}


def build(cfg, seed, stop_bias, dtype=torch.float32):
    torch.set_default_dtype(dtype)
    m = Tacotron2(num_chars=cfg.num_chars, num_speakers=cfg.num_speakers, r=cfg.r, attn_norm=cfg.attn_norm,
                  prenet_dropout=False, double_decoder_consistency=cfg.double_decoder_consistency, ddc_r=cfg.ddc_r,
                  speaker_embedding_dim=cfg.speaker_embedding_dim, prenet_type=cfg.prenet_type, gst=True,
                  gst_embedding_dim=cfg.gst_embedding_dim, gst_num_heads=cfg.gst_num_heads,
                  gst_style_tokens=cfg.gst_style_tokens, gst_use_speaker_embedding=cfg.gst_use_speaker_embedding)
    sd = synth_state_dict(tacotron2_spec(cfg), seed, GAINS)
    sd["decoder.stopnet.1.linear_layer.bias"] = np.array([stop_bias], np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval()
    if dtype == torch.float64:
        m.double()
    torch.set_default_dtype(torch.float32)
    return m


def style_mel(N, seed):
    """A (N, 80) normalised-mel-like input: a drifting ridge plus noise, within about [-4, 4]."""
    rs = np.random.RandomState(seed)
    n, c = np.meshgrid(np.arange(N), np.arange(80), indexing="ij")
    ridge = 3.0 * np.exp(-0.5 * ((c - 20 - 15 * np.sin(0.05 * n + seed)) / 9.0) ** 2) - 2.0
    return (ridge + 0.6 * rs.randn(N, 80) + 0.5 * np.sin(0.21 * n + 0.3 * seed)).astype(np.float32)


def spk_kw(spk, dtype):
    if np.ndim(spk) == 0:
        return {"speaker_ids": torch.tensor([int(spk)])}
    return {"speaker_embeddings": torch.from_numpy(np.asarray(spk)[None]).to(dtype)}


def style_embedding(m, cfg, mel, spk, dtype=torch.float32):
    """gst_layer on one mel (N, 80) -> (G,) as float64 numpy."""
    emb = None
    if cfg.gst_query_speaker_dim:
        emb = torch.from_numpy(np.asarray(spk)[None]).to(dtype)
    with torch.no_grad():
        out = m.gst_layer(torch.from_numpy(mel[None]).to(dtype), emb)
    return out.reshape(-1).double().numpy()


def dict_embedding(m, cfg, style, spk, dtype=torch.float32):
    """The style vector compute_gst concatenates for a token-weight dict -> (G,)."""
    emb = None
    if cfg.gst_query_speaker_dim:
        emb = torch.from_numpy(np.asarray(spk)[None]).to(dtype)
    torch.set_default_dtype(dtype)
    with torch.no_grad():
        out = m.compute_gst(torch.zeros(1, 1, 0).to(dtype), style, emb)
    torch.set_default_dtype(torch.float32)
    return out.reshape(-1).double().numpy()


def run_infer(m, ids, spk, style, dtype=torch.float32):
    """Reference inference of one text; style: (N, 80) mel, dict or None. Returns dec, post, align,
    stop, raw stop logits."""
    m.decoder.set_r(R)
    m.decoder.max_decoder_steps = MAX_STEPS
    logits = []
    h = m.decoder.stopnet.register_forward_hook(lambda mod, i, o: logits.append(o.detach().clone()))
    if isinstance(style, np.ndarray):
        style = torch.from_numpy(style[None]).to(dtype)
    torch.set_default_dtype(dtype)
    with torch.no_grad():
        dec, post, align, stop = m.inference(torch.from_numpy(ids[None].astype(np.int64)), style_mel=style,
                                             **spk_kw(spk, dtype))
    h.remove()
    torch.set_default_dtype(torch.float32)
    lg = torch.cat(logits, 0).reshape(-1).double().numpy()
    return (dec[0].double().numpy(), post[0].double().numpy(), align[0].double().numpy(),
            stop[0, :, 0].double().numpy(), lg)


def case(tag):
    cfg = CASES[tag]
    name = "taco_gst_" + tag
    rs = np.random.RandomState(SEEDS[tag] + 1000)
    embs = rs.randn(len(STYLE_N), 256).astype(np.float32)
    embs /= np.linalg.norm(embs, axis=1, keepdims=True)
    ext = cfg.speaker_embedding_dim is not None
    spks = [embs[i] if ext else np.int64((3, 1, 0, 2, 1)[i]) for i in range(len(STYLE_N))]
    utts = [rs.randint(1, cfg.num_chars, size=T).astype(np.int64) for T in TEXT_LENS]
    mels = {N: style_mel(N, 7 + N) for N in STYLE_N}
    sdict = STYLE_DICT[tag]
    # the inference runs: (key, text, speaker, style)
    runs = [(f"u{i}", utts[i], spks[i], mels[INFER_STYLE_N[i]]) for i in range(3)]
    runs += [("d0", utts[0], spks[0], sdict), ("z1", utts[1], spks[1], None)]

    seed = SEEDS[tag]
    for attempt in range(20):  # the first seed whose stop logits admit a bias with margin >= 1e-3
        m = build(cfg, seed, -1e4)
        raw = [run_infer(m, ids, sp, st)[4] + 1e4 for _, ids, sp, st in runs]
        best = choose_stop_bias(raw, MAX_STEPS, 1)  # as make_golden's cases: at least one run stops by its token
        if best is not None and best[1] >= 1e-3:
            break
        seed += 1
    else:
        raise SystemExit(f"[{name}] no seed with a usable stop margin")
    bias, margin = best
    print(f"[{name}] seed {seed} stop bias {bias:.6f} min margin {margin:.3e}")
    m32, m64 = build(cfg, seed, bias), build(cfg, seed, bias, torch.float64)
    out = {"cfg": json.dumps(cfg.__dict__), "overrides": json.dumps(GAINS), "seed": np.int64(seed),
           "stop_bias": np.float32(bias), "r": np.int64(R), "max_steps": np.int64(MAX_STEPS),
           "style_n": np.array(STYLE_N), "infer_style_n": np.array(INFER_STYLE_N), "style_dict": json.dumps(sdict),
           "style_spk": np.stack([np.asarray(s, np.float32 if ext else np.int64) for s in spks])}

    # style embeddings
    sdrift, styles = [], []
    for i, N in enumerate(STYLE_N):
        e32 = style_embedding(m32, cfg, mels[N], spks[i])
        e64 = style_embedding(m64, cfg, mels[N], spks[i], torch.float64)
        sdrift.append(float(np.abs(e32 - e64).max()))
        styles.append(e32)
        out[f"style_mel_{N}"] = mels[N]
        out[f"style_{N}"] = e32.astype(np.float32)
        print(f"  style N={N}: |e| {np.abs(e32).max():.3f} drift64 {sdrift[-1]:.2e}")
    d32 = dict_embedding(m32, cfg, sdict, spks[0])
    d64 = dict_embedding(m64, cfg, sdict, spks[0], torch.float64)
    sdrift.append(float(np.abs(d32 - d64).max()))
    out["dict_style"] = d32.astype(np.float32)
    style_tol = 8 * max(sdrift)
    out["style_tol"] = np.float64(style_tol)
    out["style_drift64"] = np.array(sdrift)
    # the same speaker, two mels: the embedding must depend on the mel far beyond the tolerance
    e_a = style_embedding(m32, cfg, mels[37], spks[1])
    e_b = style_embedding(m32, cfg, mels[130], spks[1])
    sep = float(np.abs(e_a - e_b).max())
    print(f"  style_tol {style_tol:.2e}, dict drift {sdrift[-1]:.2e}, two mels differ by {sep:.2e}")
    assert sep >= 1000 * style_tol, (sep, style_tol)

    # inference
    res = {}
    for key, ids, sp, st in runs:
        dec, post, align, stop, lg = run_infer(m32, ids, sp, st)
        dec64, post64 = run_infer(m64, ids, sp, st, torch.float64)[:2]
        assert len(dec) == len(dec64), key
        drift = float(max(np.abs(dec - dec64).max(), np.abs(post - post64).max()))
        assert 8 * drift <= MEL_TOL, (key, drift)
        am = np.sort(align, axis=1)
        out[key + "_ids"] = ids
        out[key + "_dec"] = dec.astype(np.float32)
        out[key + "_post"] = post.astype(np.float32)
        out[key + "_align"] = align.astype(np.float32)
        out[key + "_stop"] = stop.astype(np.float32)
        out[key + "_top2"] = (am[:, -1] - am[:, -2]).astype(np.float32)
        out[key + "_drift64"] = np.float64(drift)
        res[key] = dec
        print(f"  {key} T={len(ids)} steps={len(stop)} drift64={drift:.2e}")
    n = min(len(res["u1"]), len(res["z1"]))
    moved = float(np.abs(res["u1"][:n] - res["z1"][:n]).max())
    print(f"  a style moves the decoder output by {moved:.2e}")
    assert moved >= 50 * MEL_TOL, moved

    # eval forward: the style input is the teacher mel itself
    for i, (u, M) in enumerate(((0, 24), (2, 37))):  # M = 37: a padded last group
        ids, sp = utts[u], spks[u]
        mel = teacher_mel(res[f"u{u}"], M)
        dec, post, align, stop = run_forward(m32, ids, mel, R, spk=sp)
        dec64, post64, _, stop64 = run_forward(m64, ids, mel, R, torch.float64, spk=sp)
        drift = float(max(np.abs(dec - dec64).max(), np.abs(post - post64).max()))
        assert 8 * drift <= MEL_TOL, (i, drift)
        key = f"f{i}"
        out[key + "_ids"], out[key + "_mel"], out[key + "_M"] = ids, mel, np.int64(M)
        out[key + "_spk"] = np.asarray(sp, np.float32 if ext else np.int64)
        out[key + "_dec"], out[key + "_post"] = dec.astype(np.float32), post.astype(np.float32)
        out[key + "_align"], out[key + "_stop_logit"] = align.astype(np.float32), stop.astype(np.float32)
        out[key + "_drift64"] = np.float64(drift)
        out[key + "_stop_drift64"] = np.float64(np.abs(stop - stop64).max())
        print(f"  {key} T={len(ids)} M={M} drift64={drift:.2e} stop_drift64={float(out[key + '_stop_drift64']):.2e}")
    out["stop_tol"] = np.float64(64 * max(float(out[f"f{i}_stop_drift64"]) for i in range(2)))
    assert float(out["stop_tol"]) <= 1e-3
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] {os.path.getsize(path) / 1024:.0f} KiB")
    return [[k, list(v.shape)] for k, v in m32.state_dict().items()]


if __name__ == "__main__":
    which = sys.argv[1:] or list(CASES)
    kpath = os.path.join(HERE, "taco_gst_keys.json")
    keys = json.load(open(kpath)) if os.path.exists(kpath) else {}
    for tag in which:
        keys[tag] = case(tag)
    with open(kpath, "w") as f:
        json.dump(keys, f, indent=0)
