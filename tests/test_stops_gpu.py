"""GPU: Tacotron2 batches whose rows stop by the stopnet, at steps unrelated to their place in the
decode order (fixture taco_stops.npz: every row run alone through the reference; max_decoder_steps 32).
Early stoppers stay frozen inside live batch tiles while others run on, the tile count shrinks with
frozen and live rows below it, and one call returns status 1 for some rows and 2 for others. Every row
must equal its B = 1 truth and be exactly zero past its own stop, in every output buffer.

Bounds are those of test_gpu_parity.py's _check_taco: dec / post MEL_TOL, alignments 1e-5, stop values
1e-4, steps and statuses exact, alignment argmax exact above the stored top-2 margin."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import (STOP_SHRINK_BY, build_melgan, build_taco, load_fixture, melgan_state_dict, stop_batch,
                     stop_fixture_problems, stop_model, stop_spread_problems, stop_tags)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MEL_TOL = 1e-4
ALIGN_MARGIN = 1e-5
_truth = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    f = load_fixture("taco_stops")
    assert stop_fixture_problems(f) == []  # conditions on the reference alone, before touching the GPU
    return f


def _need(fx, tag):
    if tag not in stop_tags(fx):
        pytest.fail(f"taco_stops.npz holds no group {tag}")


def _oracle_rows(fx, tag):
    """The oracle's B = 1 run of every row of a group, computed once and shared (never modified)."""
    if tag not in _truth:
        from oracle.taco_np import TacoOracle
        cfg, sd = stop_model(fx, tag)
        orc = TacoOracle(sd, cfg.attn_norm, cfg.r)
        r, S = int(fx[tag + "_r"]), int(fx[tag + "_max_steps"])
        table = sd.get("speaker_embedding.weight")
        rows = []
        for k in range(len(fx[tag + "_lens"])):
            batch, lens, _, _, spk = stop_batch(fx, r, [k], tag)
            rows.append(orc.inference(batch[0, :lens[0]], r, S, speaker=None if spk is None else table[int(spk[0])]))
        _truth[tag] = rows
    return _truth[tag]


def _model(fx, tag):
    cfg, sd = stop_model(fx, tag)
    m = build_taco(cfg, sd)
    m.decoder.set_r(int(fx[tag + "_r"]))
    m.decoder.max_decoder_steps = int(fx[tag + "_max_steps"])
    m.decoder.verbose = False
    return m


def _run(m, fx, tag, rows):
    batch, lens, steps, status, spk = stop_batch(fx, int(fx[tag + "_r"]), rows, tag)
    kw = {} if spk is None else {"speaker_ids": torch.from_numpy(spk)}
    out = m.inference(torch.from_numpy(batch).cuda(), text_lengths=lens, **kw)
    return [t.cpu().numpy() for t in out], np.asarray(m.last_steps), np.asarray(m.last_status)


def _check_rows(fx, tag, rows, out, got_steps, got_status, label):
    """Caller row i of the call is fixture row rows[i]: steps and statuses exact, values against the
    oracle (and the stored reference arrays where the fixture has them), zero past the row's stop."""
    dec, post, align, stop = out
    r, thr = int(fx[tag + "_r"]), 0.5
    batch, lens, steps, status, _ = stop_batch(fx, r, rows, tag)
    assert stop_spread_problems(lens, steps, status, int(fx[tag + "_max_steps"]),
                                STOP_SHRINK_BY if "shrink" in label else None) == []
    assert got_steps.tolist() == steps.tolist(), f"{label}: steps"
    assert got_status.tolist() == status.tolist(), f"{label}: status"
    assert {1, 2} <= set(got_status.tolist())
    truth = _oracle_rows(fx, tag)
    stored = set(int(k) for k in fx[tag + "_stored"])
    worst = dict(dec=0.0, post=0.0, align=0.0, stop=0.0)
    for i, k in enumerate(rows):
        S, T, M = int(steps[i]), lens[i], int(steps[i]) * r
        refs = [truth[k]]
        if int(k) in stored:
            p = f"{tag}_u{int(k)}_"
            refs.append((fx[p + "dec"], fx[p + "post"], fx[p + "align"], fx[p + "stop"]))
            sel = fx[p + "top2"] > ALIGN_MARGIN
            assert np.array_equal(align[i, :S, :T].argmax(1)[sel], fx[p + "align"].argmax(1)[sel]), f"{label} row {k}: argmax"
        for d, p_, a, s in refs:
            assert len(s) == S
            e = dict(dec=np.abs(dec[i, :M] - d).max(), post=np.abs(post[i, :M] - p_).max(),
                     align=np.abs(align[i, :S, :T] - a).max(), stop=np.abs(stop[i, :S, 0] - s).max())
            for name, v in e.items():
                worst[name] = max(worst[name], float(v))
        # frozen: nothing of this row past its own stop, in any buffer
        assert not dec[i, M:].any(), f"{label} row {k}: decoder frames past the stop"
        assert not post[i, M:].any(), f"{label} row {k}: postnet frames past the stop"
        assert not align[i, S:].any(), f"{label} row {k}: alignment rows past the stop"
        assert not stop[i, S:].any(), f"{label} row {k}: stop values past the stop"
        assert not align[i, :, T:].any(), f"{label} row {k}: alignment past the text"
        assert (stop[i, S - 1, 0] > thr) == (status[i] == 1), f"{label} row {k}: last stop value vs status"
    print(f"{label}: worst |dec| {worst['dec']:.2e} |post| {worst['post']:.2e} |align| {worst['align']:.2e} "
          f"|stop| {worst['stop']:.2e}")
    assert worst["dec"] <= MEL_TOL and worst["post"] <= MEL_TOL, f"{label}: {worst}"
    assert worst["align"] <= 1e-5 and worst["stop"] <= 1e-4, f"{label}: {worst}"


@pytest.mark.parametrize("B", [17, 36, 64])
@pytest.mark.parametrize("r", [2, 1])
def test_stopnet_rows_match_their_single_runs(fx, r, B):
    """B rows in the stored scrambled caller order: 2, 3 and 4 batch tiles, each holding rows that stop
    early beside rows that run on, the last tile alive to max_decoder_steps."""
    _dev()
    tag = f"r{r}"
    _need(fx, tag)
    rows = fx[f"{tag}_order{B}"]
    out, steps, status = _run(_model(fx, tag), fx, tag, rows)
    assert out[0].shape[0] == B
    _check_rows(fx, tag, rows, out, steps, status, f"{tag} B={B}")


@pytest.mark.parametrize("r", [2, 1])
def test_caller_order_does_not_matter(fx, r):
    """The 36-row batch in two caller orders. In the second the last tile's rows all stop by step 8, so
    the relaunch at a smaller tile count starts with frozen and live rows below it."""
    _dev()
    tag = f"r{r}"
    _need(fx, tag)
    m = _model(fx, tag)
    oa, ob = fx[tag + "_order36"], fx[tag + "_order36_shrink"]
    a, sa, ta = _run(m, fx, tag, oa)
    b, sb, tb = _run(m, fx, tag, ob)
    _check_rows(fx, tag, oa, a, sa, ta, f"{tag} order36")
    _check_rows(fx, tag, ob, b, sb, tb, f"{tag} order36_shrink")
    ia, ib = np.argsort(oa), np.argsort(ob)  # back to fixture row order
    assert np.array_equal(sa[ia], sb[ib]) and np.array_equal(ta[ia], tb[ib])
    same = True
    for u, v, name in zip(a, b, ("dec", "post", "align", "stop")):
        u, v = u[ia], v[ib]
        if name == "align":  # padded to each call's own longest text: the same here
            assert u.shape == v.shape
        assert np.abs(u - v).max() <= (MEL_TOL if name in ("dec", "post") else 1e-5), name
        same = same and np.array_equal(u, v)
    print(f"{tag}: the two caller orders are {'bit-identical' if same else 'NOT bit-identical'}")


def test_stop_steps_same_in_both_gemm_modes(fx):
    """The 36-row batch on the fp32-MFMA and the split-f16 kernels: the same rows checks, so identical
    stop steps, and no range fallback."""
    from tts_amd._lib import get_engine
    _dev()
    m = _model(fx, "r2")
    rows = fx["r2_order36"]
    eng = get_engine(torch.device("cuda:0"))
    try:
        for mode in ("f32", "x3"):
            eng.set_gemm_mode(mode)
            n0 = eng.gemm_mode()[1]
            out, steps, status = _run(m, fx, "r2", rows)
            assert eng.gemm_mode() == (mode, n0)  # no range fallback
            _check_rows(fx, "r2", rows, out, steps, status, f"r2 B=36 {mode}")
    finally:
        eng.set_gemm_mode("x3")


def test_graph_decoder_stopnet_rows(fx, tmp_path):
    """The captured-graph decoder (TTS_DECODER=graph, read once per process: one child process through
    tools/taco_dump.py's stops mode) on the 17-row batch: the same row checks."""
    path = str(tmp_path / "graph.npz")
    env = dict(os.environ, TTS_DECODER="graph")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "taco_dump.py"), path, "stops"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    o = np.load(path)
    assert int(o["path"]) == 0, "the decode did not take the captured-graph path"
    _check_rows(fx, "r2", fx["r2_order17"], (o["dec"], o["post"], o["align"], o["stop"]), o["steps"], o["status"],
                "r2 B=17 graph")


def test_fused_vocoder_with_stopnet_lengths(fx):
    """inference_vocoded and the submit / finish pair on the 36-row batch (every row's steps * 2 is above
    the vocoder's minimum of 4 frames): bit-identical to inference followed by
    MultibandMelganGenerator.inference(lengths=last_mel_lengths), waveform row i zero beyond
    hop * (steps_i * r + 2 * inference padding); then two different batches pipelined through submit / finish, the second decode's
    stops happening beside the first vocoder."""
    _dev()
    m = _model(fx, "r2")
    vcfg, vsd = melgan_state_dict(3)
    voc = build_melgan(vcfg, vsd)
    r = 2

    def args(rows):
        batch, lens, steps, status, _ = stop_batch(fx, r, rows)
        assert steps.min() * r >= 4
        return torch.from_numpy(batch).cuda(), lens, steps

    def two_calls(rows):
        x, lens, steps = args(rows)
        a = m.inference(x, text_lengths=lens)
        assert m.last_steps.tolist() == steps.tolist()
        return a + (voc.inference(a[1].transpose(1, 2), lengths=m.last_mel_lengths.copy()),)

    rows_a, rows_b = fx["r2_order36"], fx["r2_order36_shrink"][::-1][:29].copy()
    for pad in (0, 2):  # the vocoder's inference padding: none, and the reference's default
        voc.inference_padding = pad
        with torch.no_grad():
            ref_a, ref_b = two_calls(rows_a), two_calls(rows_b)
            xa, la, steps_a = args(rows_a)
            xb, lb, _ = args(rows_b)
            fused = m.inference_vocoded(xa, voc, text_lengths=la)
            assert m.last_steps.tolist() == steps_a.tolist()
            fa = m.inference_vocoded_submit(xa, voc, text_lengths=la)
            fb = m.inference_vocoded_submit(xb, voc, text_lengths=lb)
            got_a, got_b = fa.result(), fb.result()
        for ref, got in ((ref_a, fused), (ref_a, got_a), (ref_b, got_b)):
            for u, v in zip(ref, got):
                assert u.shape == v.shape and torch.equal(u, v)
        wav = ref_a[4].cpu().numpy()
        for i, s in enumerate(steps_a):
            n = voc.hop * (int(s) * r + 2 * pad)
            assert wav[i, 0, :n].any() and not wav[i, 0, n:].any(), (pad, i)


def test_multispeaker_stopnet_rows(fx):
    """17 rows of taco_multispk's configuration, each with its own speaker and its own stop: per-row
    conditioning and per-row stops do not interact."""
    _dev()
    _need(fx, "spk")
    rows = fx["spk_order17"]
    out, steps, status = _run(_model(fx, "spk"), fx, "spk", rows)
    _check_rows(fx, "spk", rows, out, steps, status, "spk B=17")
