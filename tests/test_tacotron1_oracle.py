"""oracle/tacotron1_np.py pinned on the CPU: against the reference run in float64
(tests/golden/tacotron1_f64.npz), against the float32 fixtures tacotron1_*.npz, the float32 yardstick
of the new cases, and the response of dec / post to the edges the GPU tests are meant to cover."""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, taco1_case, taco1_f64, taco1_oracles, taco1_state_dict, unpack_f64
from oracle.tacotron1_np import Tacotron1Oracle
from tts_amd.spec import TacotronV1Config

MEL_TOL = 1e-4
PIN = 1e-9  # two float64 evaluations differ by ~1e-13; a float32-sized restatement error is > 1e-7
EXISTING = ("tacotron1_sigmoid", "tacotron1_softmax_last", "tacotron1_mem3", "tacotron1_linear1025")
NEW = [("q32", 1), ("q32", 3), ("q14", 1), ("q32r10", 10), ("q5r1", 1), ("last7", 7), ("last7", 2),
       ("long_sigmoid", 5), ("long_softmax", 5)]

_cache = {}


def _existing(name):
    """(fixture, cfg, {r: float64 oracle}) of one float32 fixture."""
    if name not in _cache:
        fx = np.load(os.path.join(GOLDEN, name + ".npz"))
        cfg = TacotronV1Config(**json.loads(str(fx["cfg"])))
        orc = {}
        for r in (int(v) for v in fx["r_list"]):
            sd = taco1_state_dict(cfg, int(fx[f"r{r}_seed"]), json.loads(str(fx["overrides"])), float(fx[f"r{r}_stop_bias"]))
            orc[r] = Tacotron1Oracle(sd, cfg)
        _cache[name] = (fx, cfg, orc)
    return _cache[name]


def _existing_run(name, r, i):
    key = (name, r, i)
    if key not in _cache:
        fx, _, orc = _existing(name)
        _cache[key] = orc[r].inference(fx[f"r{r}_u{i}_ids"], r, int(fx[f"r{r}_max_steps"]))
    return _cache[key]


def _existing_ids():
    out = []
    for name in EXISTING:
        fx = np.load(os.path.join(GOLDEN, name + ".npz"))
        out += [(name, int(r), i) for r in fx["r_list"] for i in range(8) if f"r{r}_u{i}_ids" in fx.files]
    return out


def _new_run(tag, r, dtype=np.float64):
    """One new case through the oracle (float64, or its float32 evaluation), computed once."""
    key = (tag, r, np.dtype(dtype).name)
    if key not in _cache:
        cfg, sd, c = taco1_case(tag)
        o64, o32 = taco1_oracles(cfg, sd)
        fx, _ = taco1_f64()
        _cache[key] = (o64 if dtype == np.float64 else o32).inference(fx[f"{tag}.ids"], r, c["max_steps"])
    return _cache[key]


def _pin(k, res, fx):
    dec, post, align, stop, logit, steps, status = res
    assert steps == fx[k + "_stop"].shape[1], f"{k}: steps {steps}"  # packed: (8, S)
    errs = {"dec": np.abs(dec - unpack_f64(fx[k + "_dec"])).max(), "align": np.abs(align - unpack_f64(fx[k + "_align"])).max(),
            "stop": np.abs(stop - unpack_f64(fx[k + "_stop"])).max()}
    if k + "_post" in fx.files:
        errs["post"] = np.abs(post - unpack_f64(fx[k + "_post"])).max()
    lg = np.abs(logit - unpack_f64(fx[k + "_logit"])).max()
    print(k, " ".join(f"{n} {e:.2e}" for n, e in errs.items()), f"logit {lg:.2e}")
    assert max(errs.values()) <= PIN
    assert lg <= PIN * max(1.0, np.abs(logit).max())  # the never-stopping cases' logits are near -1e4


@pytest.mark.parametrize("name, r, i", _existing_ids())
def test_oracle_matches_the_float64_reference_on_the_fixture_utterances(name, r, i):
    fx, _ = taco1_f64()
    res = _existing_run(name, r, i)
    _pin(f"{name}.r{r}_u{i}", res, fx)
    assert res[6] in (1, 2) and (res[6] == 1 or res[5] == int(_existing(name)[0][f"r{r}_max_steps"]) + 1)


@pytest.mark.parametrize("tag, r", NEW)
def test_oracle_matches_the_float64_reference_on_the_new_cases(tag, r):
    fx, cases = taco1_f64()
    res = _new_run(tag, r)
    _pin(f"{tag}.r{r}", res, fx)
    assert res[5] == cases[tag]["max_steps"] + 1 and res[6] == 2
    if f"{tag}.r{r}_enc" in fx.files:
        cfg, sd, _ = taco1_case(tag)
        ids = fx[f"{tag}.ids"]
        T = len(ids)
        enc = taco1_oracles(cfg, sd)[0].encoder(ids)[[0, 1, 511, 512, T - 2, T - 1]]
        assert np.abs(enc - unpack_f64(fx[f"{tag}.r{r}_enc"])).max() <= PIN


@pytest.mark.parametrize("name, r, i", _existing_ids())
def test_oracle_matches_the_float32_fixtures_within_their_own_drift(name, r, i):
    """dec and post within 1.05 x drift64 + 2^-23 max|fixture|: what the fixture's own fp32-vs-fp64
    difference and its float32 storage imply."""
    fx = _existing(name)[0]
    k = f"r{r}_u{i}"
    dec, post, _, _, _, steps, status = _existing_run(name, r, i)
    assert steps == len(fx[k + "_stop"])
    drift = float(fx[k + "_drift64"])
    for n, a in (("dec", dec), ("post", post)):
        ref = fx[f"{k}_{n}"]
        err, bound = np.abs(a - ref).max(), 1.05 * drift + 2.0 ** -23 * np.abs(ref).max()
        print(f"{name} {k} {n}: err {err:.2e} bound {bound:.2e}")
        assert err <= bound


@pytest.mark.parametrize("tag, r", NEW)
def test_float32_yardstick_of_the_new_cases(tag, r):
    """8 x e32 <= MEL_TOL: two correct float32 orders cannot differ by the tolerance the GPU tests use."""
    a, b = _new_run(tag, r), _new_run(tag, r, np.float32)
    assert b[0].dtype == np.float32 and b[1].dtype == np.float32 and a[5] == b[5]
    e32 = max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max())
    print(f"{tag} r {r}: e32 {e32:.2e}, 8 x e32 = {8 * e32:.2e}")
    assert 8 * e32 <= MEL_TOL


# ---- the edges respond: a defect confined to one of them moves dec or post by more than 10 x MEL_TOL ----
def _moved(tag, r, hook):
    cfg, sd, c = taco1_case(tag)
    fx, _ = taco1_f64()
    ref = _new_run(tag, r)
    out = taco1_oracles(cfg, sd, hook)[0].inference(fx[f"{tag}.ids"], r, c["max_steps"])
    assert out[5] == ref[5]
    return max(np.abs(out[0] - ref[0]).max(), np.abs(out[1] - ref[1]).max())


def _zero(name, sl):
    def hook(n, x):
        if n != name:
            return None
        y = x.copy()
        y[sl] = 0
        return y
    return hook


def test_the_oldest_frame_of_a_32_frame_queue_matters():
    """memory 32, r 1: the last 80 floats of the memory input are zero until step 33 (the go frames),
    so zeroing them on every step zeroes the oldest frame from the step at which it is first non-zero."""
    first = []

    def hook(n, x):
        if n != "memory":
            return None
        first.append(bool(x[-80:].any()))
        y = x.copy()
        y[-80:] = 0
        return y
    moved = _moved("q32", 1, hook)
    assert first.index(True) == 32 and len(first) == 36  # non-zero at steps 33..36 only
    print(f"oldest queue frame zeroed: moved {moved:.2e}")
    assert moved > 10 * MEL_TOL


def test_the_queue_past_its_first_1024_floats_matters():
    moved = _moved("q32", 1, _zero("memory", slice(1024, None)))
    print(f"memory input [1024:] zeroed: moved {moved:.2e}")
    assert moved > 10 * MEL_TOL


def test_the_last_position_of_a_1024_long_alignment_matters():
    moved = _moved("long_sigmoid", 5, _zero("align", slice(1023, None)))
    print(f"alpha[T - 1] left out of the context at T = 1024: moved {moved:.2e}")
    assert moved > 10 * MEL_TOL


def test_the_last_quarter_of_a_1023_long_context_sum_matters():
    moved = _moved("long_softmax", 5, _zero("align", slice(3 * 256, None)))  # the 4th slice, tc = (T + 3) / 4
    print(f"positions [768:] left out of the context at T = 1023: moved {moved:.2e}")
    assert moved > 10 * MEL_TOL


def test_the_short_rows_of_the_long_calls_keep_the_alignment_margin():
    """The rows with T = 257, 9 and 1 that share a GPU call with T = 1024: |alpha[T - 1] - 0.6| >= 1e-3
    wherever the stop rule reads it (t > T / 4), and the T = 1 row stops at step 1 by that rule."""
    fx, _ = taco1_f64()
    for tag in ("long_sigmoid", "long_softmax"):
        cfg, sd, c = taco1_case(tag)
        o = taco1_oracles(cfg, sd)[0]
        for n in c["extra"]:
            _, _, align, stop, _, steps, status = o.inference(fx[f"{tag}.ids{n}"], 5, c["max_steps"])
            t = np.arange(steps) + 1
            tested = t > n / 4
            if tested.any():
                assert np.abs(align[tested, n - 1] - 0.6).min() >= 1e-3
            assert stop.max() < 0.1
            if n == 1:
                assert steps == 1 and status == 1
