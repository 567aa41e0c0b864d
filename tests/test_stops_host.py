"""CPU: the stopnet-driven fixture (tests/golden/taco_stops.npz, made by make_stop_golden.py from the
reference) keeps the conditions its generator asserted, and the oracle reproduces its stored rows."""
import numpy as np
import pytest

from helpers import load_fixture, stop_batch, stop_fixture_problems, stop_model, stop_tags
from oracle.taco_np import TacoOracle


def test_stop_fixture_keeps_its_conditions():
    """Margin, fp64 stop steps, drift and, per stored caller order, the spread conditions: all derived
    from the stored reference data, nothing from the code under test."""
    fx = load_fixture("taco_stops")
    assert {"r2", "r1"} <= set(stop_tags(fx))
    assert stop_fixture_problems(fx) == []


@pytest.mark.parametrize("tag", ["r2", "r1", "spk"])
def test_oracle_matches_stored_stop_rows(tag):
    """The four rows stored with the reference's arrays (earliest stopper, a mid stopper, a max-steps
    row, a length-1 row): the oracle stops at the same step; frames within the amplified regime's 1e-4
    (tests/test_oracle_golden.py), alignments 1e-5, stop values 1e-4, argmax exact above the margin."""
    fx = load_fixture("taco_stops")
    if tag not in stop_tags(fx):
        pytest.fail(f"taco_stops.npz holds no group {tag}")
    r = int(fx[tag + "_r"])
    cfg, sd = stop_model(fx, tag)
    orc = TacoOracle(sd, cfg.attn_norm, cfg.r)
    table = sd.get("speaker_embedding.weight")
    for k in fx[tag + "_stored"]:
        batch, lens, steps, status, spk = stop_batch(fx, r, [k], tag)
        speaker = None if spk is None else table[int(spk[0])]
        dec, post, align, stop = orc.inference(batch[0, :lens[0]], r, int(fx[tag + "_max_steps"]), speaker=speaker)
        p = f"{tag}_u{k}_"
        assert len(stop) == steps[0] == len(fx[p + "stop"])
        assert np.abs(dec - fx[p + "dec"]).max() <= 1e-4
        assert np.abs(post - fx[p + "post"]).max() <= 1e-4
        assert np.abs(align - fx[p + "align"]).max() <= 1e-5
        assert np.abs(stop - fx[p + "stop"]).max() <= 1e-4
        sel = fx[p + "top2"] > 1e-5
        assert np.array_equal(align.argmax(1)[sel], fx[p + "align"].argmax(1)[sel])
