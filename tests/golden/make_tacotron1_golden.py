"""Generate the Tacotron (v1) parity fixtures by running the REFERENCE PyTorch CPU path.

Run by hand on a machine that has the reference checkout (``TTS_REFERENCE``, default
``/root/reference``); the tests only read the files this writes:

* ``tacotron1_keys.json``: the reference's ordered state_dict names and shapes (memory_size 5 and -1)
* ``tacotron1_*.npz``: seed, config JSON, weight gains and, per reduction factor r and utterance i,
  ``r{r}_u{i}_{ids,dec,post,align,stop,logit,top2,drift64}`` (+ ``_enc`` for utterance 1), with the
  per-r ``r{r}_seed``, ``r{r}_stop_bias`` and ``r{r}_max_steps``, in the shape of ``taco_*.npz``.
* ``tacotron1_f64.npz`` (``python make_tacotron1_golden.py f64``, which leaves the files above as they
  are): the reference run in float64 on the same utterances and on the new cases ``F64_CASES``, the
  pin of ``oracle/tacotron1_np.py``; see ``f64_file``.

Weights come from ``synth_state_dict(tacotron_spec(cfg), seed, gains)``. The stop rule of
``Decoder.inference`` (layers/tacotron.py:489-494) is: after step t, stop if t > T/4 and
(sigmoid(stop) > 0.6 or alpha[T-1] > 0.6); else stop if t > max_decoder_steps. The stopnet output is
never fed back, so one never-stopping run gives the bias-free logits, and the stop bias is then
chosen for the widest margin around logit(0.6). The conditions the issue sets are asserted below.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))

from helpers import L06, choose_bias, pack_f64  # noqa: E402
from tts_amd.spec import TacotronV1Config, tacotron_spec  # noqa: E402
from tts_amd.weights import synth_state_dict  # noqa: E402

REF = os.environ.get("TTS_REFERENCE", "/root/reference")
if REF not in sys.path:
    sys.path.insert(0, REF)

from TTS.tts.models.tacotron import Tacotron  # noqa: E402

torch.set_num_threads(8)

MEL_TOL = 1e-4
STOP_W = "decoder.stopnet.linear.weight"
STOP_B = "decoder.stopnet.linear.bias"
# per-kind weight scales: a larger stop weight widens the stop margins; the others keep every
# module sensitive to its input (the two perturbation conditions below)
GAINS = {"stop_w": 30.0, "attn_v": 4.0, "linear_tanh": 3.0, "conv": 1.5, "gru": 2.0, "linear_relu": 1.5, "linear": 1.15}


def build(cfg, sd, dtype=torch.float32):
    torch.set_default_dtype(dtype)
    m = Tacotron(num_chars=cfg.num_chars, num_speakers=0, r=cfg.r, postnet_output_dim=cfg.postnet_output_dim,
                 attn_norm=cfg.attn_norm, memory_size=cfg.memory_size)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval()
    if dtype == torch.float64:
        m.double()
    torch.set_default_dtype(torch.float32)
    return m


def run(m, ids, r, max_steps, dtype=torch.float32):
    """(dec, post, align, stop, stopnet inputs, encoder output) of one utterance, as float64 arrays."""
    m.decoder.set_r(r)
    m.decoder.max_decoder_steps = max_steps
    sin = []
    h = m.decoder.stopnet.register_forward_pre_hook(lambda mod, i: sin.append(i[0].detach().clone()))
    torch.set_default_dtype(dtype)  # Decoder._init_states creates default-dtype state
    try:
        with torch.no_grad(), open(os.devnull, "w") as null:
            x = torch.from_numpy(ids[None].astype(np.int64))
            enc = m.encoder(m.embedding(x))
            out, sys.stdout = sys.stdout, null
            try:
                dec, post, align, stop = m.inference(x)
            finally:
                sys.stdout = out
    finally:
        h.remove()
        torch.set_default_dtype(torch.float32)
    return (dec[0].double().numpy(), post[0].double().numpy(), align[0].double().numpy(),
            stop[0, :, 0].double().numpy(), torch.cat(sin, 0).double().numpy(), enc[0].double().numpy())


def case(name, cfg, seed, utt_lens, r_list, max_steps, min_token_stops, need_max_row, id_seed, gains=None):
    gains = dict(gains or GAINS)
    rs = np.random.RandomState(id_seed)
    utts = [rs.randint(1, cfg.num_chars, size=T).astype(np.int64) for T in utt_lens]
    out = {"cfg": json.dumps(cfg.__dict__), "r_list": np.array(r_list), "overrides": json.dumps(gains)}
    spec = tacotron_spec(cfg)
    totals = {"token": 0, "max": 0, "bank": 0.0, "gru": 0.0}
    # one model per file: the seed and the stop bias are shared by every r (set_r between calls)
    ms0 = max_steps[r_list[0]]
    assert all(max_steps[r] == ms0 for r in r_list)
    for attempt in range(40):
        sd = synth_state_dict(spec, seed, gains)
        sd[STOP_B] = np.array([-1e4], np.float32)  # never stops by the token
        m = build(cfg, sd)
        w = sd[STOP_W].astype(np.float64)[0]
        raw, aligns = [], []
        for r in r_list:
            for ids in utts:
                _, _, al, _, sin, _ = run(m, ids, r, ms0)
                raw.append(sin @ w)
                aligns.append(al)
        best = choose_bias(raw, list(utt_lens) * len(r_list), aligns, ms0, min_token_stops, need_max_row)
        if best is not None and best[1] >= 1e-2:
            break
        seed += 1
    else:
        raise SystemExit(f"[{name}] no seed with a usable stop margin")
    b, margin, ntok, nmax = best
    print(f"[{name}] seed {seed} stop bias {b:.6f} min margin {margin:.3e} token stops {ntok} max rows {nmax}")
    for r in r_list:
        out["seed"] = seed
        out[f"r{r}_seed"] = np.int64(seed)
        out[f"r{r}_stop_bias"] = np.float32(b)
        out[f"r{r}_max_steps"] = np.int32(max_steps[r])
        sd[STOP_B] = np.array([b], np.float32)
        m32, m64 = build(cfg, sd), build(cfg, sd, torch.float64)
        # perturbed copies: one bank convolution scaled by 1.001, one element of a decoder GRUCell's W_hh
        sd_bank = dict(sd)
        sd_bank["postnet.cbhg.conv1d_banks.2.conv1d.weight"] = sd["postnet.cbhg.conv1d_banks.2.conv1d.weight"] * np.float32(1.001)
        sd_gru = dict(sd)
        wg = sd["decoder.decoder_rnns.0.weight_hh"].copy()
        wg[300, 7] += np.float32(0.25)
        sd_gru["decoder.decoder_rnns.0.weight_hh"] = wg
        m_bank, m_gru = build(cfg, sd_bank), build(cfg, sd_gru)
        moved = {"bank": 0.0, "gru": 0.0}
        for i, ids in enumerate(utts):
            T = len(ids)
            dec, post, align, stop, sin, enc = run(m32, ids, r, max_steps[r])
            dec64, post64, _, _, _, _ = run(m64, ids, r, max_steps[r], torch.float64)
            assert len(dec) == len(dec64), f"[{name}] fp32 and fp64 step counts differ"
            drift = max(float(np.abs(dec - dec64).max()), float(np.abs(post - post64).max()))
            assert 8 * drift <= MEL_TOL, f"[{name}] drift64 {drift:.2e} too large for MEL_TOL"
            lg = sin @ sd[STOP_W].astype(np.float64)[0] + b
            S = len(stop)
            t = np.arange(S) + 1
            tested = t > T / 4
            assert np.abs(lg[tested] - L06).min() >= 1e-2
            assert np.abs(align[tested, T - 1] - 0.6).min() >= 1e-3
            by_tok = bool(lg[-1] > L06 and tested[-1])
            by_al = bool(align[-1, T - 1] > 0.6 and tested[-1])
            if T == 1:
                assert S == 1 and by_al and not by_tok, "the T = 1 utterance stops at step 1 by the alignment rule"
            totals["token"] += by_tok and not by_al
            if not by_tok and not by_al:
                assert S == max_steps[r] + 1 and max_steps[r] <= 24
                totals["max"] += 1
            for key, mp in (("bank", m_bank), ("gru", m_gru)):
                p2 = run(mp, ids, r, max_steps[r])[1]
                if len(p2) == len(post):
                    moved[key] = max(moved[key], float(np.abs(p2 - post).max()))
            am = np.sort(align, axis=1)
            top2 = am[:, -1] - am[:, -2] if align.shape[1] > 1 else np.full(len(align), np.inf)
            k = f"r{r}_u{i}"
            out[f"{k}_ids"] = ids
            out[f"{k}_dec"] = dec.astype(np.float32)
            out[f"{k}_post"] = post.astype(np.float32)
            out[f"{k}_align"] = align.astype(np.float32)
            out[f"{k}_stop"] = stop.astype(np.float32)
            out[f"{k}_logit"] = lg.astype(np.float32)
            out[f"{k}_top2"] = top2.astype(np.float32)
            out[f"{k}_drift64"] = np.float64(drift)
            if i == min(1, len(utts) - 1):
                out[f"{k}_enc"] = enc.astype(np.float32)
            print(f"  utt{i} T={T} steps={S} frames={len(dec)} token={by_tok} align={by_al} drift64={drift:.2e} "
                  f"|post|max={np.abs(post).max():.2f}")
        print(f"  post moved by: bank conv x1.001 {moved['bank']:.2e}, one W_hh element {moved['gru']:.2e}")
        totals["bank"] = max(totals["bank"], moved["bank"])
        totals["gru"] = max(totals["gru"], moved["gru"])
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] {os.path.getsize(path) / 1024:.0f} KiB")
    return totals


def keys_file():
    out = {}
    for ms in (5, -1):
        m = Tacotron(num_chars=129, num_speakers=0, r=5, postnet_output_dim=1025, memory_size=ms)
        out[f"memory_size_{ms}"] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "tacotron1_keys.json"), "w") as f:
        json.dump(out, f, indent=0)


# ---- tacotron1_f64.npz: the reference in float64 (the pin of oracle/tacotron1_np.py) ----
EXISTING = ("tacotron1_sigmoid", "tacotron1_softmax_last", "tacotron1_mem3", "tacotron1_linear1025")
NEVER = -1e4  # stop bias of the new cases: the token never stops a row
# (tag, memory_size, r_init, attn_norm, r run, T, max_steps, first seed); T > 4 (max_steps + 1), so the
# stop rule is never evaluated. What each exercises in tacotron1.hip is in tests/test_tacotron1_edges_gpu.py.
F64_CASES = [
    ("q32", 32, 5, "sigmoid", [1, 3], 150, 35, 51),
    ("q14", 14, 5, "sigmoid", [1], 100, 20, 52),
    ("q32r10", 32, 10, "sigmoid", [10], 40, 8, 53),
    ("q5r1", 5, 1, "sigmoid", [1], 30, 6, 54),
    ("last7", -1, 7, "softmax", [7, 2], 60, 6, 55),
    ("long_sigmoid", 5, 5, "sigmoid", [5], 1024, 5, 56),
    ("long_softmax", 5, 5, "softmax", [5], 1023, 5, 57),
]
LONG_EXTRA = {"long_sigmoid": (257, 9, 1), "long_softmax": (257,)}  # the other rows of the ragged GPU calls (ids only)
# utterances whose post is stored (129-wide); the others are left out to keep the file under 500 KB
F64_POST = {"tacotron1_sigmoid.r5_u0", "tacotron1_sigmoid.r5_u1", "tacotron1_sigmoid.r2_u0", "tacotron1_sigmoid.r2_u1",
            "tacotron1_softmax_last.r5_u0", "q5r1.r1", "last7.r2"}
_grid = pack_f64


def f64_file():
    """tests/golden/tacotron1_f64.npz: the reference's float64 outputs (dec, align, stop, logit) for
    every (file, r, utterance) of the four float32 fixtures, keyed ``{file}.r{r}_u{i}_*``, and for the
    new cases F64_CASES, keyed ``{tag}.r{r}_*`` with ``{tag}.ids``. The two long cases hold encoder
    rows {0, 1, 511, 512, T-2, T-1} (``_enc``) and no post. Weights are regenerated from the stored
    seeds and gains.

    Size: raw float64 arrays of all of this take 1 MB, so (a) every array is stored as helpers.pack_f64
    does, fixed point in multiples of 2^-38 (a rounding error of 1.8e-12, against the 1e-9 the oracle is
    held to), read back with helpers.unpack_f64; (b) post is stored for the utterances in F64_POST only:
    of the 129-wide models' utterances it is left out for tacotron1_sigmoid r5 u2 / u3 and r2 u2 / u3,
    tacotron1_softmax_last u1, tacotron1_mem3 u0 / u1, q32 (r 1 and 3), q14, q32r10 and last7 r 7. The
    float32 fixtures pin the oracle's post for every one of their utterances to their own drift64."""
    out = {}

    def store(k, res):
        dec, po, align, stop, sin, enc = res
        out[k + "_dec"], out[k + "_align"], out[k + "_stop"] = _grid(dec), _grid(align), _grid(stop)
        if k in F64_POST:
            out[k + "_post"] = _grid(po)

    for name in EXISTING:
        fx = np.load(os.path.join(HERE, name + ".npz"))
        cfg = TacotronV1Config(**json.loads(str(fx["cfg"])))
        for r in (int(v) for v in fx["r_list"]):
            sd = synth_state_dict(tacotron_spec(cfg), int(fx[f"r{r}_seed"]), json.loads(str(fx["overrides"])))
            sd[STOP_B] = np.array([float(fx[f"r{r}_stop_bias"])], np.float32)
            m64 = build(cfg, sd, torch.float64)
            i = 0
            while f"r{r}_u{i}_ids" in fx.files:
                res = run(m64, fx[f"r{r}_u{i}_ids"], r, int(fx[f"r{r}_max_steps"]), torch.float64)
                assert len(res[3]) == len(fx[f"r{r}_u{i}_stop"]), "the float64 run stops elsewhere"
                k = f"{name}.r{r}_u{i}"
                store(k, res)
                out[k + "_logit"] = _grid(res[4] @ sd[STOP_W].astype(np.float64)[0] + np.float64(sd[STOP_B][0]))
                i += 1
    cases = []
    for tag, mem, r_init, norm, r_list, T, ms, seed in F64_CASES:
        cfg = TacotronV1Config(memory_size=mem, r=r_init, attn_norm=norm, postnet_output_dim=129)
        assert T > 4 * (ms + 1)
        rs = np.random.RandomState(1000 + seed)
        ids = rs.randint(1, cfg.num_chars, size=T).astype(np.int64)
        extra = {n: rs.randint(1, cfg.num_chars, size=n).astype(np.int64) for n in LONG_EXTRA.get(tag, ())}
        long = tag in LONG_EXTRA
        for attempt in range(20):
            sd = synth_state_dict(tacotron_spec(cfg), seed, GAINS)
            sd[STOP_B] = np.array([NEVER], np.float32)
            m32, m64 = build(cfg, sd), build(cfg, sd, torch.float64)
            runs, drift, ok = {}, 0.0, True
            for r in r_list:
                a, b = run(m32, ids, r, ms), run(m64, ids, r, ms, torch.float64)
                assert len(a[3]) == len(b[3]) == ms + 1
                drift = max(drift, float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))
                runs[r] = b
            for n, x in extra.items():  # rows that do reach the alignment rule: the fixtures' margin
                al = run(m64, x, r_list[0], ms, torch.float64)[2]
                t = np.arange(len(al)) + 1
                ok &= bool(np.abs(al[t > n / 4, n - 1] - 0.6).min() >= 1e-3) if (t > n / 4).any() else True
            if 8 * drift <= MEL_TOL and ok:
                break
            seed += 1
        else:
            raise SystemExit(f"[{tag}] no seed with 8 x drift64 <= MEL_TOL")
        print(f"[{tag}] seed {seed} drift64 {drift:.2e} (8 x = {8 * drift:.2e})")
        out[f"{tag}.ids"] = ids
        for n, x in extra.items():
            out[f"{tag}.ids{n}"] = x
        for r in r_list:
            store(f"{tag}.r{r}", runs[r])
            out[f"{tag}.r{r}_logit"] = _grid(runs[r][4] @ sd[STOP_W].astype(np.float64)[0] + NEVER)
            if long:
                out[f"{tag}.r{r}_enc"] = _grid(runs[r][5][[0, 1, 511, 512, T - 2, T - 1]])
        cases.append({"tag": tag, "cfg": cfg.__dict__, "seed": seed, "r_list": r_list, "max_steps": ms,
                      "stop_bias": NEVER, "extra": list(extra)})
    out["cases"] = json.dumps(cases)
    out["overrides"] = json.dumps(GAINS)
    path = os.path.join(HERE, "tacotron1_f64.npz")
    np.savez_compressed(path, **out)
    print(f"[tacotron1_f64] {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    keys_file()
    tot = {"token": 0, "max": 0, "bank": 0.0, "gru": 0.0}

    def add(t):
        for k in ("token", "max"):
            tot[k] += t[k]
        for k in ("bank", "gru"):  # largest move of a stored post under each perturbation
            tot[k] = max(tot[k], t[k])

    add(case("tacotron1_sigmoid", TacotronV1Config(memory_size=5, r=5, attn_norm="sigmoid", postnet_output_dim=129),
             seed=11, utt_lens=[1, 9, 23, 40], r_list=[5, 2], max_steps={5: 12, 2: 12}, min_token_stops=1,
             need_max_row=True, id_seed=101))
    add(case("tacotron1_softmax_last",
             TacotronV1Config(memory_size=-1, r=5, attn_norm="softmax", postnet_output_dim=129),
             seed=21, utt_lens=[7, 18], r_list=[5], max_steps={5: 10}, min_token_stops=1, need_max_row=False,
             id_seed=102))
    add(case("tacotron1_mem3", TacotronV1Config(memory_size=3, r=5, attn_norm="sigmoid", postnet_output_dim=129),
             seed=31, utt_lens=[11, 16], r_list=[5], max_steps={5: 10}, min_token_stops=0, need_max_row=False,
             id_seed=103))
    add(case("tacotron1_linear1025", TacotronV1Config(memory_size=5, r=5, attn_norm="sigmoid", postnet_output_dim=1025),
             seed=41, utt_lens=[6], r_list=[5], max_steps={5: 3}, min_token_stops=0, need_max_row=False,
             id_seed=104, gains=dict(GAINS, linear=1.3)))  # a 1025-wide last_linear has a smaller xavier bound
    assert tot["token"] >= 2, "at least two utterances stop by the stop token"
    assert tot["max"] >= 1, "at least one utterance reaches max_decoder_steps"
    assert tot["bank"] > 10 * MEL_TOL and tot["gru"] > 10 * MEL_TOL, "outputs do not respond to the weights"
    print("token stops", tot["token"], "max-steps rows", tot["max"])


if __name__ == "__main__":
    if sys.argv[1:] == ["f64"]:  # the float64 file alone; the four float32 fixtures stay as they are
        f64_file()
    else:
        main()
