"""Tacotron (v1) on the GPU at the limits include/ttship.h states, against oracle/tacotron1_np.py
(float64, pinned to the reference by tests/test_tacotron1_oracle.py):

* memory queues whose shift passes one and two 1024-float slots of t1_decoder_kernel's keep[3]
  (nkeep = (memory_size - r) 80 = 2480, 2320, 1040, 1760), r_init 10, 1 and 7 (proj_to_mel split over
  S = 1024 / (20 r_init) = 5, 51 and 7 slices of K), the prenet GEMV at K = 2560;
* rows of 1024 and 1023 positions (attention energy loop, both normalisations, the four-slice context
  sum, 1024 GRU steps, 128 conv tiles) in a ragged call with rows of 257, 9 and 1;
* 64 rows that stop by the token, by the alignment rule and at max_decoder_steps, and 65 rows;
* the postnet alone at lengths around a tile, 129 and 1025 wide; the four fences.

Tolerances are those of test_tacotron1_gpu.py's _check. Every comparison prints its error beside the
float32 yardstick e32 = max|oracle(float32) - oracle(float64)| and their ratio before it asserts; the
CPU tests hold 8 x e32 <= 1e-4 for the fixture's cases, so two correct float32 orders cannot differ by
the tolerance."""
import json

import numpy as np
import pytest
import torch

from helpers import L06, build_taco1, choose_bias, taco1_case, taco1_f64, taco1_oracles, taco1_state_dict, unpack_f64
from tts_amd.spec import TacotronV1Config

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4
ALIGN_TOL = 1e-5
ALIGN_MARGIN = 1e-5

_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _model(key, cfg, sd):
    """One loaded model per configuration."""
    _dev()
    m = _cached(("model", key), lambda: build_taco1(cfg, sd))
    m.decoder.verbose = False
    return m


def _oracle_run(o, ids, r, ms):
    enc = o.encoder(ids)
    dec, align, stop, logit, steps, status = o.decoder_inference(enc, r, ms)
    return dict(enc=enc, dec=dec, post=o.postnet(dec), align=align, stop=stop, logit=logit, steps=steps, status=status)


def _ref(key, cfg, sd, ids, r, ms):
    """(float64 oracle run, float32 oracle run) of one utterance, computed once."""
    def make():
        o64, o32 = taco1_oracles(cfg, sd)
        return _oracle_run(o64, ids, r, ms), _oracle_run(o32, ids, r, ms)
    return _cached(("ref", key, len(ids), r, ms), make)


def _infer(m, rows, r, ms):
    """rows: id arrays; ms: max_decoder_steps per row -> numpy (dec, post, align, stop), steps, status."""
    m.decoder.set_r(r)
    lens = [len(x) for x in rows]
    batch = np.zeros((len(rows), max(lens)), np.int64)
    for j, x in enumerate(rows):
        batch[j, :len(x)] = x
    out = m.inference(torch.from_numpy(batch).cuda(), text_lengths=lens, max_decoder_steps=np.asarray(ms))
    return [t.cpu().numpy() for t in out], m.last_steps.copy(), m.last_status.copy()


def _report(what, err, e32):
    print(f"{what}: err {err:.3e} e32 {e32:.3e} ratio {err / max(e32, 1e-30):.2f}")


def _check_row(what, out, j, steps, status, ref, ref32, r):
    """Row j of a call against its oracle run: the checks of _check in test_tacotron1_gpu.py."""
    dec, post, align, stop = out
    S, T = ref["steps"], ref["align"].shape[1]
    assert steps[j] == S and status[j] == ref["status"], f"{what}: steps {steps[j]} status {status[j]}, oracle {S} {ref['status']}"
    M = S * r
    same = ref32["steps"] == S
    for n, a in (("dec", dec), ("post", post)):
        err = np.abs(a[j, :M] - ref[n]).max()
        _report(f"{what} {n}", err, np.abs(ref32[n] - ref[n]).max() if same else np.nan)
    ea, es = np.abs(align[j, :S, :T] - ref["align"]).max(), np.abs(stop[j, :S, 0] - ref["stop"]).max()
    print(f"{what}: steps {S} align err {ea:.3e} stop err {es:.3e}")
    assert np.abs(dec[j, :M] - ref["dec"]).max() <= MEL_TOL and np.abs(post[j, :M] - ref["post"]).max() <= MEL_TOL
    assert ea <= ALIGN_TOL and es <= MEL_TOL
    assert not dec[j, M:].any() and not post[j, M:].any()
    assert not align[j, S:].any() and not align[j, :, T:].any() and not stop[j, S:].any()
    if T > 1:
        top = np.sort(ref["align"], axis=1)
        sel = top[:, -1] - top[:, -2] > ALIGN_MARGIN
        assert np.array_equal(align[j, :S, :T].argmax(1)[sel], ref["align"].argmax(1)[sel])


def _align_margin(ref, T):
    """|alpha[T - 1] - 0.6| over the steps at which the stop rule reads it (t > T / 4)."""
    t = np.arange(ref["steps"]) + 1
    tested = t > T / 4
    return np.abs(ref["align"][tested, T - 1] - 0.6).min() if tested.any() else np.inf


# ---- 1. memory queues and r_init ----
SMALL = [("q32", 1), ("q32", 3), ("q14", 1), ("q32r10", 10), ("q5r1", 1), ("last7", 7), ("last7", 2)]


@pytest.mark.parametrize("tag, r", SMALL)
def test_queue_and_r_init_configurations(tag, r):
    cfg, sd, c = taco1_case(tag)
    fx, _ = taco1_f64()
    ids, ms = fx[f"{tag}.ids"], c["max_steps"]
    T = len(ids)
    m = _model(tag, cfg, sd)
    ref, ref32 = _ref(tag, cfg, sd, ids, r, ms)
    # the oracle run is the fixture's (the reference in float64)
    assert np.abs(ref["dec"] - unpack_f64(fx[f"{tag}.r{r}_dec"])).max() <= 1e-9
    out, steps, status = _infer(m, [ids], r, [ms])
    _check_row(f"{tag} r {r} alone", out, 0, steps, status, ref, ref32, r)
    # a second row, shorter in T and longer in steps: neither row is the call's maximum in both
    ids2 = np.random.RandomState(7).randint(1, cfg.num_chars, size=T - 3).astype(np.int64)
    second, second32 = _ref(tag + "/second", cfg, sd, ids2, r, ms + 2)
    assert second["steps"] == ms + 3 and _align_margin(second, T - 3) >= 1e-3
    out2, steps, status = _infer(m, [ids, ids2], r, [ms, ms + 2])
    _check_row(f"{tag} r {r} row 0 of 2", out2, 0, steps, status, ref, ref32, r)
    _check_row(f"{tag} r {r} row 1 of 2", out2, 1, steps, status, second, second32, r)
    assert np.array_equal(out2[0][0, :steps[0] * r], out[0][0]) and np.array_equal(out2[1][0, :steps[0] * r], out[1][0])


# ---- 2. long rows ----
def _long_rows(tag, lens):
    fx, _ = taco1_f64()
    src = {1024: "long_sigmoid.ids", 1023: "long_softmax.ids"}
    return [fx[src[n]] if n in src else fx[f"{tag}.ids{n}"] for n in lens]


@pytest.mark.parametrize("tag, lens", [("long_sigmoid", [1024, 1023, 257, 9, 1]), ("long_softmax", [1023, 257])])
def test_long_rows_in_a_ragged_call(tag, lens):
    cfg, sd, c = taco1_case(tag)
    assert c["stop_bias"] == -1e4 and c["max_steps"] == 5 and cfg.r == 5
    rows = _long_rows(tag, lens)
    m = _model(tag, cfg, sd)
    refs = [_ref(tag, cfg, sd, ids, 5, 5) for ids in rows]
    for (ref, _), n in zip(refs, lens):
        assert _align_margin(ref, n) >= 1e-3
        if n == 1 or n > 24:  # T = 1 stops at step 1 by the alignment rule; the long rows never reach the rule
            assert (ref["steps"], ref["status"]) == ((1, 1) if n == 1 else (6, 2))
    batch = np.zeros((len(rows), max(lens)), np.int64)
    for j, x in enumerate(rows):
        batch[j, :len(x)] = x
    enc = m.encode(torch.from_numpy(batch).cuda(), lens).cpu().numpy()
    for j, n in enumerate(lens):
        err = np.abs(enc[j, :n] - refs[j][0]["enc"]).max()
        _report(f"{tag} encoder T {n}", err, np.abs(refs[j][1]["enc"] - refs[j][0]["enc"]).max())
        assert err <= MEL_TOL and not enc[j, n:].any()
    out, steps, status = _infer(m, rows, 5, [5] * len(rows))
    for j, n in enumerate(lens):
        _check_row(f"{tag} T {n}", out, j, steps, status, refs[j][0], refs[j][1], 5)
    for j, n in enumerate(lens):  # a fixed order per row: each row equals its own B = 1 call bit for bit
        one, s1, _ = _infer(m, [rows[j]], 5, [5])
        S = int(s1[0])
        assert S == steps[j]
        assert np.array_equal(one[0][0], out[0][j, :S * 5]) and np.array_equal(one[1][0], out[1][j, :S * 5])
        assert np.array_equal(one[2][0], out[2][j, :S, :n]) and np.array_equal(one[3][0], out[3][j, :S])


# ---- 3. 64 rows stopped by the rule ----
B64_SEED, B64_LENS, B64_R, B64_MS = 71, (1, 5, 9, 16, 23, 31, 40, 64), 2, 14


def _b64():
    """cfg, state dict with the chosen stop bias, the 8 utterances and their oracle runs."""
    def make():
        fx, _ = taco1_f64()
        gains = json.loads(str(fx["overrides"]))
        cfg = TacotronV1Config(memory_size=5, r=5, attn_norm="sigmoid", postnet_output_dim=129)
        rs = np.random.RandomState(B64_SEED)
        utts = [rs.randint(1, cfg.num_chars, size=T).astype(np.int64) for T in B64_LENS]
        # the stopnet output is never fed back: one run that the token never stops gives the bias-free logits
        free = taco1_oracles(cfg, taco1_state_dict(cfg, B64_SEED, gains, -1e4))[0]
        runs = [free.decoder_inference(free.encoder(ids), B64_R, B64_MS) for ids in utts]
        raw = [run[3] + 1e4 for run in runs]
        best = choose_bias(raw, list(B64_LENS), [run[1] for run in runs], B64_MS, 3, True)
        assert best is not None, "no stop bias with three token stops and a row at max_decoder_steps"
        bias = float(np.float32(best[0]))
        sd = taco1_state_dict(cfg, B64_SEED, gains, bias)
        return cfg, sd, utts, [_ref("b64", cfg, sd, ids, B64_R, B64_MS) for ids in utts]
    return _cached("b64", make)


def b64_conditions(refs):
    """The conditions on the oracle alone, every utterance included: (token stops' steps, rows stopped
    by the alignment rule, rows at max_decoder_steps + 1 steps, min stop margin, min alignment margin)."""
    tok, ali, mx, m_stop, m_al = [], 0, 0, np.inf, np.inf
    for (ref, _), T in zip(refs, B64_LENS):
        S = ref["steps"]
        t = np.arange(S) + 1
        tested = t > T / 4
        if tested.any():
            m_stop = min(m_stop, np.abs(ref["logit"][tested] - L06).min())
            m_al = min(m_al, np.abs(ref["align"][tested, T - 1] - 0.6).min())
        by_tok, by_al = tested[-1] and ref["logit"][-1] > L06, tested[-1] and ref["align"][-1, T - 1] > 0.6
        if by_tok and not by_al:
            tok.append(S)
        elif by_al:
            ali += 1
        else:
            assert S == B64_MS + 1 and ref["status"] == 2
            mx += 1
    return tok, ali, mx, m_stop, m_al


def test_sixty_four_rows_stopped_by_the_rule():
    cfg, sd, utts, refs = _b64()
    tok, ali, mx, m_stop, m_al = b64_conditions(refs)
    print(f"64 rows: token stops at steps {tok}, alignment stops {ali}, max rows {mx}, margins {m_stop:.2e} {m_al:.2e}")
    assert len(tok) >= 3 and len(set(tok)) >= 3 and ali >= 1 and mx >= 1
    assert m_stop >= 1e-2 and m_al >= 1e-3
    m = _model("b64", cfg, sd)
    order = np.random.RandomState(64).permutation(np.repeat(np.arange(8), 8))
    out, steps, status = _infer(m, [utts[i] for i in order], B64_R, [B64_MS] * 64)
    first = {}
    for j, i in enumerate(order):
        _check_row(f"b64 row {j} (T {B64_LENS[i]})", out, j, steps, status, refs[i][0], refs[i][1], B64_R)
        if i in first:  # the copies of an utterance are bit-identical
            assert all(np.array_equal(a[j], a[first[i]]) for a in out)
        first.setdefault(i, j)
    # 65 rows go through two library calls
    out65, steps65, status65 = _infer(m, [utts[i] for i in order] + [utts[3]], B64_R, [B64_MS] * 65)
    assert np.array_equal(steps65[:64], steps) and np.array_equal(status65[:64], status)
    assert all(np.array_equal(a[:64], b) for a, b in zip(out65, out))
    assert all(np.array_equal(a[64], a[first[3]]) for a in out65)


# ---- 4. the postnet stage alone ----
POST_LENS = [1, 7, 8, 9, 203]


@pytest.mark.parametrize("width", [129, 1025])
def test_postnet_stage_alone(width):
    fx, _ = taco1_f64()
    cfg, sd, _ = taco1_case("q5r1", postnet_output_dim=width)
    m = _model(("q5r1", width), cfg, sd)
    # oracle decoder frames (the fixture's float64 dec is the oracle's to 1e-9)
    pool = np.concatenate([unpack_f64(fx[k]) for k in ("q32.r3_dec", "q32r10.r10_dec", "q32.r1_dec")])
    offs = np.concatenate([[0], np.cumsum(POST_LENS)])
    assert offs[-1] <= len(pool)
    rows = [pool[a:b] for a, b in zip(offs[:-1], offs[1:])]
    batch = np.zeros((len(rows), max(POST_LENS), 80), np.float32)
    for j, d in enumerate(rows):
        batch[j, :len(d)] = d
    post = m.run_postnet(torch.from_numpy(batch).cuda(), POST_LENS).cpu().numpy()
    assert post.shape == (5, 203, width)
    o64, o32 = taco1_oracles(cfg, sd)
    for j, n in enumerate(POST_LENS):
        ref = o64.postnet(batch[j, :n])  # the float32 frames the kernel was given
        err = np.abs(post[j, :n] - ref).max()
        _report(f"postnet {width} row {j} ({n} frames)", err, np.abs(o32.postnet(batch[j, :n]) - ref).max())
        assert err <= MEL_TOL
        assert not post[j, n:].any()


# ---- 5. the fences ----
def _still_matches(what):
    cfg, sd, c = taco1_case("q5r1")
    ids = taco1_f64()[0]["q5r1.ids"]
    ref, ref32 = _ref("q5r1", cfg, sd, ids, 1, c["max_steps"])
    out, steps, status = _infer(_model("q5r1", cfg, sd), [ids], 1, [c["max_steps"]])
    _check_row(f"after {what}", out, 0, steps, status, ref, ref32, 1)


def test_fence_input_positions():
    cfg, sd, _ = taco1_case("q5r1")
    m = _model("q5r1", cfg, sd)
    m.decoder.set_r(1)
    with pytest.raises(RuntimeError, match="more than 1024 input positions"):
        m.inference(torch.ones(1, 1025, dtype=torch.long).cuda(), max_decoder_steps=2)
    _still_matches("T = 1025")


@pytest.mark.parametrize("changes, message", [(dict(r=11), r"r must be in \[1, 10\]"),
                                              (dict(memory_size=33), "memory_size above 32")])
def test_fence_model_limits(changes, message):
    _dev()
    cfg, _, c = taco1_case("q5r1", **changes)
    bad = build_taco1(cfg, taco1_state_dict(cfg, c["seed"], {}, -1e4))
    with pytest.raises(RuntimeError, match=message):
        bad.inference(torch.ones(1, 8, dtype=torch.long).cuda(), max_decoder_steps=2)
    _still_matches(str(changes))


def test_fence_set_r_above_r_init():
    cfg, sd, _ = taco1_case("q5r1")
    m = _model("q5r1", cfg, sd)
    m.decoder.set_r(cfg.r + 1)
    with pytest.raises(ValueError, match=r"r=2 must be in \[1, r_init=1\]"):
        m.inference(torch.ones(1, 8, dtype=torch.long).cuda(), max_decoder_steps=2)
    _still_matches("set_r(r_init + 1)")
