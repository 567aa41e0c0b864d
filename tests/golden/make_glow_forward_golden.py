"""Generate the Glow-TTS analysis fixtures by running the REFERENCE ``GlowTts.forward`` on the CPU.

Run where the reference checkout is (``TTS_REFERENCE``, as for make_golden.py), from the repository
root; no GPU is needed:

    python tests/golden/make_glow_forward_golden.py [glow_fwd] [glow_fwd_spk]

``forward(x, x_lengths, y, y_lengths)`` in ``eval()`` (``TTS/tts/models/glow_tts.py:114-156``) is the
analysis direction: forward flows (``z``, ``logdet``), the likelihood matrix ``logp``, the monotonic
alignment search and the outputs along the found path. Every row is run alone (B = 1), in fp32 and
again with ``.double()``; ``logp`` is what the reference hands to its ``maximum_path``. The teacher mel
of a row is the same model's ``inference`` output for the row's ids, cut or zero-extended to the
row's Ty frames, plus ``0.25 sin(0.37 n + 0.11 c)`` (as make_teacher_golden.py). Only seeds, ids,
mels, outputs and the recorded drifts are stored, never weights.

    glow_fwd.npz      the ``glow`` fixture's model (gated-conv encoder, single speaker)
    glow_fwd_spk.npz  the ``glow_spk_tfm`` fixture's model (transformer encoder, 3 speakers,
                      c_in 64), rows under speakers 2 and 0 in turn

Rows (Tx, Ty): (1, 2) one token, the smallest even length; (5, 11) an odd length trimmed to 10;
(8, 8) the path forced onto the diagonal; (70, 150) more than one wave of tokens, more than two
64-frame tiles, the band clipped on both sides.

Path stability is a condition on the fixture: over the backtrack decisions of the reference's search
(``monotonic_align/core.pyx:32-35``) ``margin`` is the smallest ``|Q[i, y-1] - Q[i-1, y-1]|`` that was
compared, and ``qdrift`` the largest difference between the fp32 and the fp64 run's ``Q``. A row's
data seed is accepted only if ``margin >= 10 * qdrift`` (tried in order from the row's base seed);
both numbers are stored and the condition is asserted, so an implementation whose ``logp`` is as
close to the exact one as the reference's fp32 run finds the same path.

``glow_fwd.npz`` also records the round trip on the ``glow`` fixture's utterance u1: the reference's
``forward`` on its own noise-free ``inference`` mel. The row meets the margin condition, but the
search cannot give back ``inference``'s durations there: 18 of u1's 31 tokens have ``w_ceil = 0``
(no frame in ``generate_path``), and a monotonic path gives every token at least one frame. So
``rt_ok`` (the row is stable AND the reference's search returns ``w_ceil``) is 0, and the GPU test
compares against ``rt_dur``, the frames per token the reference's ``forward`` finds on that mel; it
compares against ``rt_w_ceil`` too only when ``rt_ok`` is 1. The margin condition itself is asserted
for this row as for the others.
"""

import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_glow_tts  # noqa: E402
from tts_amd.spec import GlowConfig, glow_spec  # noqa: E402
from tts_amd.weights import synth_state_dict  # noqa: E402

ROWS = ((1, 2), (5, 11), (8, 8), (70, 150))
MARGIN_FACTOR = 10.0
NEG = -1e9


def build(cfg, seed):
    GlowTts = import_glow_tts()
    m = GlowTts(num_chars=cfg.num_chars, hidden_channels=192, filter_channels=768, filter_channels_dp=256,
                out_channels=80, kernel_size=3, num_heads=2, num_layers_enc=6, encoder_type=cfg.encoder_type,
                dropout_p=0.1, num_flow_blocks_dec=12, kernel_size_dec=5, dilation_rate=1, num_block_layers=4,
                dropout_p_dec=0.05, num_speakers=cfg.num_speakers, c_in_channels=cfg.c_in_channels, num_splits=4,
                num_sqz=2, sigmoid_scale=False, mean_only=True, hidden_channels_enc=192, hidden_channels_dec=192,
                use_encoder_prenet=True)
    sd = synth_state_dict(glow_spec(cfg), seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.eval()


def q_table(logp, tx, ty, dtype):
    """The recurrence of maximum_path_each (core.pyx:17-30) in ``dtype``; cells outside the band stay NaN."""
    v = logp.astype(dtype)
    q = np.full((tx, ty), np.nan, dtype)
    neg = dtype(NEG)
    for y in range(ty):
        for x in range(max(0, tx + y - ty), min(tx, y + 1)):
            v_cur = neg if x == y else q[x, y - 1]
            v_prev = (dtype(0) if y == 0 else neg) if x == 0 else q[x - 1, y - 1]
            q[x, y] = max(v_cur, v_prev) + v[x, y]
    return q


def backtrack(q, tx, ty):
    """core.pyx:32-35 on a Q table: the path (tx, ty) and the smallest compared difference."""
    path = np.zeros((tx, ty), np.uint8)
    index, margin = tx - 1, np.inf
    for y in range(ty - 1, -1, -1):
        path[index, y] = 1
        if index != 0:
            if index != y:
                margin = min(margin, abs(float(q[index, y - 1]) - float(q[index - 1, y - 1])))
            if index == y or q[index, y - 1] < q[index - 1, y - 1]:
                index -= 1
    return path, margin


def run_forward(m, glow_mod, ids, mel, spk, dtype):
    """Reference forward on one row; returns (z, logdet, logp, attn (Ty, Tx), o_attn_dur (Tx), y_mean,
    o_dur_log (Tx)) as float64."""
    seen = {}
    orig = glow_mod.maximum_path

    def spy(value, mask):
        seen["logp"] = value.detach().clone()
        return orig(value, mask)

    glow_mod.maximum_path = spy
    try:
        with torch.no_grad():
            g = None if spk is None else torch.tensor([int(spk)])
            out = m.forward(torch.from_numpy(ids[None]), torch.tensor([len(ids)]),
                            torch.from_numpy(mel[None]).to(dtype), torch.tensor([mel.shape[1]]), g=g)
    finally:
        glow_mod.maximum_path = orig
    z, logdet, y_mean, y_log_scale, attn, o_dur_log, o_attn_dur = out
    assert not y_log_scale.any()
    return (z[0].double().numpy(), float(logdet[0]), seen["logp"][0].double().numpy(), attn[0].double().numpy(),
            o_attn_dur[0, 0].double().numpy(), y_mean[0].double().numpy(), o_dur_log[0, 0].double().numpy())


def teacher_mel(m, ids, spk, Ty):
    """The model's own inference mel cut or zero-extended to Ty frames, plus a sinusoid."""
    with torch.no_grad():
        torch.manual_seed(7)
        g = None if spk is None else torch.tensor([int(spk)])
        y = m.inference(torch.from_numpy(ids[None]), torch.tensor([len(ids)]), g=g)[0][0].numpy()
    mel = np.zeros((80, Ty), np.float64)
    n = min(Ty, y.shape[1])
    mel[:, :n] = y[:, :n]
    cc, nn = np.meshgrid(np.arange(80), np.arange(Ty), indexing="ij")
    return (mel + 0.25 * np.sin(0.37 * nn + 0.11 * cc)).astype(np.float32)


def analyse(m32, m64, glow_mod, ids, mel, spk):
    """Both reference runs of one row, the search restated on their logp, and the stability numbers."""
    tx, ty = len(ids), mel.shape[1] // 2 * 2
    z, logdet, logp, attn, dur, ymean, logw = run_forward(m32, glow_mod, ids, mel, spk, torch.float32)
    z64, logdet64, logp64 = run_forward(m64, glow_mod, ids, mel, spk, torch.float64)[:3]
    assert z.shape == (80, ty) and logp.shape == (tx, ty) and attn.shape == (ty, tx)
    q32 = q_table(logp, tx, ty, np.float32)
    q64 = q_table(logp64, tx, ty, np.float64)
    path, margin = backtrack(q32, tx, ty)
    assert np.array_equal(path.T, attn), "the restated search does not reproduce the reference's path"
    band = ~np.isnan(q32)
    qdrift = float(np.abs(q32[band].astype(np.float64) - q64[band]).max())
    return {"z": z, "z64": z64, "logdet": logdet, "logdet64": logdet64, "logp": logp, "logp64": logp64,
            "path": path, "dur": dur, "ymean": ymean, "logw": logw, "margin": float(margin), "qdrift": qdrift}


def store_row(out, key, ids, mel, spk, data_seed, r):
    out[key + "_ids"] = ids
    out[key + "_mel"] = mel
    out[key + "_data_seed"] = np.int64(data_seed)
    if spk is not None:
        out[key + "_spk"] = np.int64(spk)
    out[key + "_z64"] = r["z64"]
    out[key + "_logdet64"] = np.float64(r["logdet64"])
    out[key + "_logp"] = r["logp"].astype(np.float32)  # the fp32 run's own matrix: what its search saw
    out[key + "_logp64"] = r["logp64"]
    out[key + "_attn"] = r["path"].T.copy()  # (Ty, Tx) as forward returns it
    out[key + "_oattn_dur"] = r["dur"].astype(np.float32)
    out[key + "_ymean"] = r["ymean"].astype(np.float32)
    out[key + "_logw"] = r["logw"].astype(np.float32)
    out[key + "_z_drift"] = np.float64(np.abs(r["z"] - r["z64"]).max())
    out[key + "_logp_drift"] = np.float64(np.abs(r["logp"] - r["logp64"]).max())
    out[key + "_logdet_drift"] = np.float64(abs(r["logdet"] - r["logdet64"]))
    out[key + "_margin"] = np.float64(r["margin"])
    out[key + "_qdrift"] = np.float64(r["qdrift"])


def save_npz(path, out):
    """np.savez_compressed with fixed member timestamps, so a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in out:
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(out[k]), allow_pickle=False)


def forward_case(name, src_name, base_seed, speakers=None):
    import_glow_tts()  # builds the reference's Cython search before its package is imported
    import TTS.tts.models.glow_tts as glow_mod
    src = np.load(os.path.join(HERE, src_name + ".npz"))
    num_speakers = int(src["num_speakers"]) if "num_speakers" in src.files else 0
    c_in = int(src["c_in"]) if "c_in" in src.files else 0
    cfg = GlowConfig(encoder_type=str(src["encoder_type"]), num_speakers=num_speakers, c_in_channels=c_in)
    seed = int(src["seed"])
    m32 = build(cfg, seed)
    m64 = build(cfg, seed).double()
    out = {"seed": np.int64(seed), "encoder_type": str(src["encoder_type"]), "num_speakers": np.int64(num_speakers),
           "c_in": np.int64(c_in), "source": "GlowTts.forward", "rows": np.array(ROWS, np.int64),
           "margin_factor": np.float64(MARGIN_FACTOR)}
    for i, (tx, ty) in enumerate(ROWS):
        spk = None if speakers is None else speakers[i % len(speakers)]
        for attempt in range(20):
            data_seed = base_seed + 100 * i + attempt
            ids = np.random.RandomState(data_seed).randint(1, cfg.num_chars, size=tx).astype(np.int64)
            mel = teacher_mel(m32, ids, spk, ty)
            r = analyse(m32, m64, glow_mod, ids, mel, spk)
            ok = r["margin"] >= MARGIN_FACTOR * r["qdrift"]
            print(f"  [{name}] u{i} (Tx {tx}, Ty {ty}) seed {data_seed}: margin {r['margin']:.3e} qdrift "
                  f"{r['qdrift']:.3e} {'accepted' if ok else 'rejected'}")
            if ok:
                break
        assert r["margin"] >= MARGIN_FACTOR * r["qdrift"], (name, i)
        store_row(out, f"u{i}", ids, mel, spk, data_seed, r)
        print(f"  [{name}] u{i}: drifts z {out[f'u{i}_z_drift']:.2e} logp {out[f'u{i}_logp_drift']:.2e} "
              f"logdet {out[f'u{i}_logdet_drift']:.2e} (logdet {r['logdet64']:.4f})")
    if speakers is None:
        round_trip(out, src, m32, m64, glow_mod)
    path = os.path.join(HERE, name + ".npz")
    save_npz(path, out)
    print(f"[{name}] {os.path.getsize(path) / 1024:.0f} KiB")


def round_trip(out, src, m32, m64, glow_mod):
    """forward on the noise-free inference mel of the ``glow`` fixture's u1: does the search give back
    inference's durations, and does the row meet the margin condition?"""
    ids = src["u1_ids"]
    old = m32.noise_scale
    m32.noise_scale = 0.0
    with torch.no_grad():
        y, _, _, _, attn, _, _ = m32.inference(torch.from_numpy(ids[None]), torch.tensor([len(ids)]))
    m32.noise_scale = old
    w_ceil = attn[0].sum(0).numpy()  # frames per token of generate_path
    mel = y[0].numpy()
    even = mel.shape[1] % 2 == 0 and mel.shape[1] == attn.shape[1]
    r = analyse(m32, m64, glow_mod, ids, mel, None) if mel.shape[1] >= max(2, len(ids)) else None
    same = bool(r is not None and even and np.array_equal(r["path"].sum(1), w_ceil))
    stable = bool(r is not None and r["margin"] >= MARGIN_FACTOR * r["qdrift"])
    assert r is not None and even and stable
    out["rt_ok"] = np.int64(same and stable)
    out["rt_dur"] = r["path"].sum(1).astype(np.float32)
    out["rt_w_ceil"] = w_ceil.astype(np.float32)
    out["rt_margin"] = np.float64(r["margin"] if r else np.nan)
    out["rt_qdrift"] = np.float64(r["qdrift"] if r else np.nan)
    print(f"  [round trip] glow u1 Tx {len(ids)} Ty {mel.shape[1]}: same durations {same}, margin "
          f"{out['rt_margin']:.3e} qdrift {out['rt_qdrift']:.3e} -> rt_ok {int(out['rt_ok'])}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["glow_fwd", "glow_fwd_spk"]
    if "glow_fwd" in which:
        forward_case("glow_fwd", "glow", base_seed=5100)
    if "glow_fwd_spk" in which:
        forward_case("glow_fwd_spk", "glow_spk_tfm", base_seed=6100, speakers=(2, 0))
