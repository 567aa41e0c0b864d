"""Host-side checks of ``GlowTts.forward`` (no GPU): the alignment fixtures (tests/golden/
make_glow_forward_golden.py) are reproduced by a numpy restatement of the reference's search and
meet their path-stability condition; the library declares and exports the two new entry points;
``forward`` raises where it has to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import load_fixture
from tts_amd import GlowTts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("glow_fwd", "glow_fwd_spk")
ROWS = ((1, 2), (5, 11), (8, 8), (70, 150))


def maximum_path_each(value, t_x, t_y, max_neg_val=-1e9):
    """``monotonic_align/core.pyx:9-35`` in numpy float32: ``value`` (t_x, t_y) -> path (t_x, t_y)."""
    value = value.astype(np.float32).copy()
    neg = np.float32(max_neg_val)
    for y in range(t_y):
        for x in range(max(0, t_x + y - t_y), min(t_x, y + 1)):
            v_cur = neg if x == y else value[x, y - 1]
            v_prev = (np.float32(0) if y == 0 else neg) if x == 0 else value[x - 1, y - 1]
            value[x, y] = max(v_cur, v_prev) + value[x, y]
    path = np.zeros((t_x, t_y), np.int32)
    index = t_x - 1
    for y in range(t_y - 1, -1, -1):
        path[index, y] = 1
        if index != 0 and (index == y or value[index, y - 1] < value[index - 1, y - 1]):
            index -= 1
    return path


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_rows_and_restated_search(name):
    fx = load_fixture(name)
    assert [tuple(r) for r in fx["rows"]] == list(ROWS)
    for i, (tx, ty) in enumerate(ROWS):
        k = f"u{i}"
        te = ty // 2 * 2
        assert len(fx[k + "_ids"]) == tx and fx[k + "_mel"].shape == (80, ty)
        assert fx[k + "_logp"].shape == (tx, te) and fx[k + "_logp"].dtype == np.float32
        assert fx[k + "_attn"].shape == (te, tx) and fx[k + "_z64"].shape == (80, te)
        path = maximum_path_each(fx[k + "_logp"], tx, te)
        assert np.array_equal(path.T, fx[k + "_attn"]), (name, k)
        # one token per frame, every token at least once, monotonic
        assert (path.sum(0) == 1).all() and (path.sum(1) >= 1).all()
        assert np.allclose(fx[k + "_oattn_dur"], np.log(1 + path.sum(1)), atol=1e-6)
    diag = fx["u2_attn"]
    assert np.array_equal(diag, np.eye(8))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_paths_are_stable(name):
    """margin >= 10 x the fp32-vs-fp64 drift of Q on every committed row (the generator's condition)."""
    fx = load_fixture(name)
    assert float(fx["margin_factor"]) == 10.0
    for i in range(len(ROWS)):
        margin, qdrift = float(fx[f"u{i}_margin"]), float(fx[f"u{i}_qdrift"])
        assert qdrift > 0 and margin >= 10.0 * qdrift, (name, i, margin, qdrift)
        for q in ("z", "logp", "logdet"):
            assert float(fx[f"u{i}_{q}_drift"]) > 0
    if name == "glow_fwd":
        assert float(fx["rt_margin"]) >= 10.0 * float(fx["rt_qdrift"])
        assert fx["rt_dur"].sum() == fx["rt_w_ceil"].sum() and (fx["rt_dur"] >= 1).all()


def test_entry_points_declared_typed_and_exported():
    from tts_amd._lib import LIB_PATH, SIGNATURES
    header = open(os.path.join(ROOT, "include", "ttship.h")).read()
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("tts_glow_align", "tts_glow_mas"):
        assert re.search(r"\bint %s\(tts_ctx\* ctx" % name, header)
        assert name in {n for n, _, _ in SIGNATURES}
        assert hasattr(lib, name)


def _args(B=2, T=6, Ty=12):
    return torch.ones(B, T, dtype=torch.long), torch.full((B,), T), torch.zeros(B, 80, Ty)


def test_forward_raises_on_cpu_in_train_and_without_a_mel():
    m = GlowTts(num_chars=130).eval()
    x, xl, y = _args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward(x, xl, y, torch.tensor([12, 8]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, xl, y)
    with pytest.raises(AttributeError, match="size"):  # the reference's y.size(2) on None
        m.forward(x, xl)
    m.train()
    with pytest.raises(NotImplementedError, match="training forward"):
        m.forward(x, xl, y)
    with pytest.raises(NotImplementedError, match="training forward"):
        m.forward(x, xl)


def test_forward_speaker_misuse_fails_as_inference():
    x, xl, y = _args(B=1)
    with pytest.raises(AttributeError, match="emb_g"):
        GlowTts(num_chars=130).eval().forward(x, xl, y, g=torch.tensor([0]))
    with pytest.raises(AttributeError, match="cond_layer"):
        GlowTts(num_chars=130, num_speakers=4).eval().forward(x, xl, y, g=torch.tensor([0]))
    m = GlowTts(num_chars=130, num_speakers=4, c_in_channels=36).eval()
    with pytest.raises(RuntimeError, match="pass g"):
        m.forward(x, xl, y)
    with pytest.raises(IndexError):
        m.forward(x, xl, y, g=torch.tensor([4]))
