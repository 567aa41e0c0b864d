"""oracle/voc_np.py pinned on the CPU: its float64 form against the same operations written with
torch.nn.functional in float64, its float32 form against oracle/melgan_np.py (the float32 restatement of
the reference generator, itself pinned to the reference's recorded outputs) layer by layer on the mbmelgan
fixture's weights."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import load_fixture, melgan_oracle, melgan_state_dict
from oracle import melgan_np as M
from oracle import voc_np as V
from oracle.taco_np import conv1d


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _weights(rs, C, dils):
    blocks = []
    for d in dils:
        blocks.append((rs.normal(0, 1 / np.sqrt(3 * C), (C, C, 3)).astype(np.float32), rs.normal(0, 0.5, C).astype(np.float32),
                       rs.normal(0, 1 / np.sqrt(C), (C, C, 1)).astype(np.float32), rs.normal(0, 0.5, C).astype(np.float32),
                       rs.normal(0, 1 / np.sqrt(C), (C, C, 1)).astype(np.float32), rs.normal(0, 0.5, C).astype(np.float32), d))
    return blocks


def _torch_block(x, wd, bd, w1, b1, ws, bs, d):
    h = F.conv1d(F.pad(F.leaky_relu(x, 0.2), (d, d), mode="reflect"), _t(wd), _t(bd), dilation=d)
    return F.conv1d(x, _t(ws), _t(bs)) + F.conv1d(F.leaky_relu(h, 0.2), _t(w1), _t(b1))


@pytest.mark.parametrize("C, dils, L", [(32, (1, 3, 9), 40), (48, (27,), 28), (48, (14, 1, 1), 17), (96, (9, 3, 1), 33)])
def test_float64_blocks_equal_torch(C, dils, L):
    rs = np.random.RandomState(C + L)
    blocks = _weights(rs, C, dils)
    x = rs.normal(0, 1, (C, L)).astype(np.float32)
    y, mx = V.resstack(x, blocks)
    t = _t(x)[None]
    seen = float(np.abs(x).max())
    for blk in blocks:
        d = blk[6]
        h = F.conv1d(F.pad(F.leaky_relu(t, 0.2), (d, d), mode="reflect"), _t(blk[0]), _t(blk[1]), dilation=d)
        seen = max(seen, float(t.abs().max()), float(h.abs().max()))
        t = _torch_block(t, *blk)
    assert np.abs(y - t[0].numpy()).max() <= 1e-12 * max(1.0, float(t.abs().max()))
    assert abs(mx - seen) <= 1e-12 * seen
    y1, mx1 = V.resblock(x, *blocks[0])
    assert np.abs(y1 - _torch_block(_t(x)[None], *blocks[0])[0].numpy()).max() <= 1e-12 * max(1.0, float(np.abs(y1).max()))
    # a batch is its rows
    x2 = rs.normal(0, 1, (C, L + 5)).astype(np.float32)
    yb, mxb = V.resstack([x, x2], blocks)
    assert np.abs(yb[0] - y).max() <= 1e-12 * max(1.0, float(np.abs(y).max())) and yb[1].shape == (C, L + 5) and mxb >= mx


@pytest.mark.parametrize("Lin", [1, 9, 30])
def test_float64_conv_transpose_stack_equals_torch(Lin):
    C = 48
    rs = np.random.RandomState(Lin)
    blocks = _weights(rs, C, (1, 3, 9) if Lin >= 9 else (1, 1, 1))
    ct_w = rs.normal(0, 1 / np.sqrt(4 * C), (2 * C, C, 4)).astype(np.float32)
    ct_b = rs.normal(0, 0.5, C).astype(np.float32)
    xin = rs.normal(0, 1, (2 * C, Lin)).astype(np.float32)
    x0 = F.conv_transpose1d(F.leaky_relu(_t(xin)[None], 0.2), _t(ct_w), _t(ct_b), stride=2, padding=1)
    assert x0.shape == (1, C, 2 * Lin)
    assert np.abs(V.conv_transpose2(xin, ct_w, ct_b) - x0[0].numpy()).max() <= 1e-12 * max(1.0, float(x0.abs().max()))
    if Lin < 9:  # rows of 2: shorter than the first block's reflection needs from dilation 2 on
        return
    y, mx = V.ct_resstack(xin, ct_w, ct_b, blocks)
    t = x0
    for blk in blocks:
        t = _torch_block(t, *blk)
    assert np.abs(y - t[0].numpy()).max() <= 1e-12 * max(1.0, float(t.abs().max()))
    assert mx >= float(np.abs(xin).max()) and mx >= float(x0.abs().max()) * (1 - 1e-12)


@pytest.mark.parametrize("C, N, L", [(32, 4, 4), (48, 4, 21), (64, 1, 37)])
def test_float64_output_stage_equals_torch(C, N, L):
    from tts_amd.pqmf import pqmf_filters
    rs = np.random.RandomState(C + L)
    wo = rs.normal(0, 1 / np.sqrt(7 * C), (N, C, 7)).astype(np.float32)
    bo = rs.normal(0, 0.5, N).astype(np.float32)
    x = rs.normal(0, 1, (C, L)).astype(np.float32)
    b, mx = V.out_bands(x, wo, bo)
    tb = torch.tanh(F.conv1d(F.pad(F.leaky_relu(_t(x)[None], 0.2), (3, 3), mode="reflect"), _t(wo), _t(bo)))
    assert np.abs(b - tb[0].numpy()).max() <= 1e-13 and mx == float(np.abs(x).max())
    if N != 4:
        return
    G = np.asarray(pqmf_filters()[1], np.float32).reshape(4, -1)
    taps = G.shape[1] - 1
    y, _ = V.out_pqmf(x, wo, bo, G)
    up = torch.zeros(4, 4, 4, dtype=torch.float64)
    for k in range(4):
        up[k, k, 0] = 4.0
    ty = F.conv1d(F.conv_transpose1d(tb, up, stride=4), _t(G)[None], padding=taps // 2)  # pqmf.py:51-56
    assert y.shape == (1, 4 * L) and np.abs(y - ty[0].numpy()).max() <= 1e-13


def test_float32_chain_is_conv_np_chain_sum():
    """voc_np.chain_sum32 (blocked, threaded) against conv_np.chain_sum: one block, several, a ragged last."""
    from oracle import conv_np as O
    rs = np.random.RandomState(5)
    w = rs.normal(0, 1, (24, 19, 3)).astype(np.float32)
    for n in (0, 1, 1023, 1024, 1025, 3 * 1024 + 7):
        g = rs.normal(0, 1, (19, 3, n)).astype(np.float32)
        assert np.array_equal(V.chain_sum32(w, g), O.chain_sum(w, g, np.float32))


def _close32(what, mine32, mine64, theirs):
    """Two float32 evaluations of one expression (a term-by-term chain here, a blocked matrix product there):
    each lies within its own rounding error of the float64 value. The chain's error e32 is measured; a
    blocked product's partial sums are no longer than the chain's, so 2 x e32 bounds the distance. One float32
    spacing at the output scale is added for the results' own final roundings (and for tanh / the bias sum)."""
    e32 = float(np.abs(mine32.astype(np.float64) - mine64).max())
    scale = max(1.0, float(np.abs(mine64).max()))
    d = float(np.abs(mine32.astype(np.float64) - theirs).max())
    print(f"{what}: |float32 form - melgan_np| {d:.3e}, e32 {e32:.3e}")
    assert mine32.dtype == np.float32 and d <= 2 * e32 + 2 ** -23 * scale, what


@pytest.mark.parametrize("key", ["M7_p0", "M5_p2"])
def test_float32_form_equals_melgan_oracle_layer_by_layer(key):
    """Every layer runs on melgan_np's own activation, so no error carries from one layer to the next."""
    fx = load_fixture("mbmelgan")
    cfg, sd = melgan_state_dict(int(fx["seed"]))
    orc = melgan_oracle(cfg, sd)
    pad = int(key.split("_p")[1])
    mel = np.asarray(fx[key + "_mel"][0], np.float32)
    c = np.concatenate([np.repeat(mel[:, :1], pad, 1), mel, np.repeat(mel[:, -1:], pad, 1)], 1) if pad else mel
    ls, w, b = orc.layers, orc.w, orc.b
    x = conv1d(M.reflect_pad(c, ls[0].padding), w[ls[0].name], b[ls[0].name])
    i, nstage = 1, 0
    while i < len(ls) and ls[i].kind == "convT":
        l = ls[i]
        xn = M.conv_transpose1d(M.leaky_relu(x), w[l.name], b[l.name], l.stride, l.padding, l.extra.get("output_padding", 0))
        if l.stride == 2:
            _close32(f"stage {nstage} ConvTranspose", V.conv_transpose2(x, w[l.name], b[l.name], np.float32),
                     V.conv_transpose2(x, w[l.name], b[l.name]), xn)
        x = xn
        i += 1
        blocks = []
        while i < len(ls) and ls[i].kind == "res_dconv":
            dc, pw, sc = ls[i], ls[i + 1], ls[i + 2]
            blk = (w[dc.name], b[dc.name], w[pw.name], b[pw.name], w[sc.name], b[sc.name], dc.dilation)
            h = conv1d(M.reflect_pad(M.leaky_relu(x), dc.padding), w[dc.name], b[dc.name], dilation=dc.dilation)
            h = conv1d(M.leaky_relu(h), w[pw.name], b[pw.name])
            xn = (conv1d(x, w[sc.name], b[sc.name]) + h).astype(np.float32)
            _close32(f"stage {nstage} block {len(blocks)}", V.resblock(x, *blk, np.float32)[0], V.resblock(x, *blk)[0], xn)
            blocks.append(blk)
            x = xn
            i += 3
        nstage += 1
    l = ls[i]
    bands = np.tanh(conv1d(M.reflect_pad(M.leaky_relu(x), l.padding), w[l.name], b[l.name])).astype(np.float32)
    _close32("output conv", V.out_bands(x, w[l.name], b[l.name], np.float32)[0], V.out_bands(x, w[l.name], b[l.name])[0], bands)
    G = np.asarray(orc.G, np.float32).reshape(bands.shape[0], -1)
    wav = M.pqmf_synthesis(bands, orc.G)
    _close32("PQMF synthesis", V.pqmf_synthesis(bands, G, np.float32), V.pqmf_synthesis(bands, G), wav)
    # the whole generator and inference, as the class runs them
    assert np.array_equal(orc.generator(c), bands) and np.array_equal(orc.inference(mel, pad), wav)
    assert nstage == len(cfg.upsample_factors)
