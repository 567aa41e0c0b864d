"""CPU: oracle/conv_np.py (the float64 statement of the generic conv, the reference of
tests/test_conv_edges_gpu.py) against torch float64 on the CPU, to 1e-12 relative: F.conv1d over F.pad
(zero / reflect / replicate), F.conv_transpose1d for the definition and for both descriptions of it
(polyphase, phase-merged), and the epilogue forms written out."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_np as O

REL = 1e-12


def _close(a, b, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= REL * max(1.0, np.abs(b).max() if b.size else 1.0), f"{what}: {err:.3e}"


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _torch_conv(x, w, bias, dil, left, right, mode):
    xp = F.pad(_t(x)[None], (left, right), mode={0: "constant", 1: "reflect", 2: "replicate"}[mode])
    return F.conv1d(xp, _t(w), _t(bias), dilation=dil)[0].numpy()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("K, dil", [(1, 1), (2, 1), (2, 7), (3, 1), (3, 3), (5, 1), (7, 1)])
def test_conv1d_matches_torch_over_padding(mode, K, dil):
    rs = np.random.RandomState(K * 10 + dil + mode)
    span = (K - 1) * dil
    w, bias = rs.normal(size=(5, 16, K)), rs.normal(size=5)
    for pad_left in sorted({0, span // 2, span}):
        for L in (span + 1, 23):
            x = rs.normal(size=(16, L))
            got = O.conv_rows([x], w, bias, [L], dil=dil, pad_left=(pad_left,), pad_mode=mode)[0]
            # the library's convs keep the length: right padding = span - pad_left
            _close(got, _torch_conv(x, w, bias, dil, pad_left, span - pad_left, mode), f"K {K} pad {pad_left} L {L}")


def test_short_rows_zero_and_clamp_and_a_batch():
    rs = np.random.RandomState(3)
    w, bias = rs.normal(size=(4, 16, 7)), rs.normal(size=4)
    xs = [rs.normal(size=(16, L)) for L in (1, 2, 9)]
    for mode in (0, 2):
        got = O.conv_rows(xs, w, bias, [1, 2, 9], pad_left=(3,), pad_mode=mode)
        for x, g in zip(xs, got):
            _close(g, _torch_conv(x, w, bias, 1, 3, 3, mode), f"mode {mode} L {x.shape[1]}")


def test_rep_pad_is_replicate_then_reflect():
    """The vocoder's first conv: replicate padding of the mel by rep_pad, ReflectionPad1d(3), k7."""
    rs = np.random.RandomState(4)
    w, bias, x = rs.normal(size=(6, 16, 7)), rs.normal(size=6), rs.normal(size=(16, 9))
    got = O.conv_rows([x], w, bias, [9], pad_left=(3,), pad_mode=1, rep_pad=2, len_add=4)[0]
    xp = F.pad(F.pad(_t(x)[None], (2, 2), mode="replicate"), (3, 3), mode="reflect")
    _close(got, F.conv1d(xp, _t(w), _t(bias))[0].numpy())
    assert got.shape == (6, 13)


def test_activation_on_load_and_float32_form():
    rs = np.random.RandomState(5)
    w, bias, x = rs.normal(size=(3, 32, 3)), rs.normal(size=3), rs.normal(size=(32, 11))
    got = O.conv_rows([x], w, bias, [11], pad_left=(1,), act=1)[0]
    _close(got, _torch_conv(F.leaky_relu(_t(x), 0.2).numpy(), w, bias, 1, 1, 1, 0))
    g32 = O.conv_rows([x.astype(np.float32)], w.astype(np.float32), bias.astype(np.float32), [11], pad_left=(1,), act=1,
                      dtype=np.float32)[0]
    assert g32.dtype == np.float32
    e = np.abs(g32 - got).max()
    assert 0 < e < 1e-4  # a float32 evaluation: close, and not the float64 one


@pytest.mark.parametrize("u", [2, 4, 8])
def test_conv_transpose_three_ways(u):
    rs = np.random.RandomState(u)
    Cin, Cout, L = 16, 5, 7
    wt, bias, x = rs.normal(size=(Cin, Cout, 2 * u)), rs.normal(size=Cout), rs.normal(size=(Cin, L))
    ref = F.conv_transpose1d(F.leaky_relu(_t(x), 0.2)[None], _t(wt), _t(bias), stride=u, padding=u // 2)[0].numpy()
    assert ref.shape == (Cout, L * u)
    _close(O.conv_transpose1d(x, wt, bias, u, act=1), ref, "definition")
    Wm, pls = O.convT_polyphase(wt, u)
    _close(O.conv_rows([x], Wm, bias, [L], pad_left=pls, out_mul=u, act=1)[0], ref, "polyphase")
    _close(O.convT_merged(x, wt, bias, u, act=1), ref, "merged")


def test_epilogues_written_out():
    rs = np.random.RandomState(9)
    Cout, T = 8, 6
    z = rs.normal(size=(Cout, T))
    tz = _t(z)
    r = rs.normal(size=(Cout, T))
    _close(O.epilogue(z, 1, np.float64, resid=r), (torch.relu(tz) + _t(r)).numpy(), "relu + residual")
    got = O.epilogue(z, 2, np.float64, resid=r, resid_rows=3)
    want = torch.tanh(tz).numpy()
    want[:3] += r[:3]
    _close(got, want, "tanh + residual rows")
    u, g = tz[0::2], tz[1::2]
    _close(O.epilogue(z, 3, np.float64), (torch.tanh(u) * torch.sigmoid(g)).numpy(), "gate")
    a = rs.normal(size=Cout)
    ta = _t(a)
    _close(O.epilogue(z, 3, np.float64, aux=a),
           (torch.tanh(u + ta[0::2, None]) * torch.sigmoid(g + ta[1::2, None])).numpy(), "gate + aux")
    _close(O.epilogue(z, 6, np.float64), F.glu(torch.cat([u, g]), dim=0).numpy(), "glu")
    x = rs.normal(size=(Cout // 2, T))
    _close(O.epilogue(z, 4, np.float64, resid=x), ((_t(x) - u) * torch.exp(-g)).numpy(), "coupling")
    # form 5: x = [x0; x1] (Cout channels), x1' = (x1 - m) exp(-logs), then per group of
    # {x0[2m], x0[2m + 1], x1'[2m], x1'[2m + 1]} the 4 x 4 mix of the table's rows, (v - bias) * scale
    x = rs.normal(size=(Cout, T))
    tab = rs.normal(size=(Cout, 6))
    Ch = Cout // 2
    x1 = (x[Ch:] - z[0::2]) * np.exp(-z[1::2])
    want = np.zeros((Cout, T))
    for m in range(0, Ch, 2):
        grp = np.stack([x[m], x[m + 1], x1[m], x1[m + 1]])
        for c in (m, m + 1, Ch + m, Ch + m + 1):
            want[c] = (tab[c, :4] @ grp - tab[c, 4]) * tab[c, 5]
    _close(O.epilogue(z, 5, np.float64, resid=x, aux=tab), want, "coupling + invconv + actnorm")


def test_polyphase_out_mul_and_residual_through_conv_rows():
    rs = np.random.RandomState(11)
    w, bias = rs.normal(size=(4, 6, 16, 2)), rs.normal(size=6)
    xs = [rs.normal(size=(16, L)) for L in (5, 3)]
    res = [rs.normal(size=(6, 4 * L)) for L in (5, 3)]
    got = O.conv_rows(xs, w, bias, [5, 3], pad_left=(1, 1, 0, 0), out_mul=4, resid=res, resid_rows=2)
    for x, r, g in zip(xs, res, got):
        want = np.zeros_like(g)
        for ph in range(4):
            left = (1, 1, 0, 0)[ph]
            want[:, ph::4] = _torch_conv(x, w[ph], bias, 1, left, 1 - left, 0)
        want[:2] += r[:2]
        _close(g, want)
