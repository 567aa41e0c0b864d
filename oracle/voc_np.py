"""The vocoder's fused kernels (tts_amd/csrc/resblock.hip, resblock_x3.hip, resstack_x3.hip, melgan_out.hip)
in plain numpy on top of oracle/conv_np.py, at float64 or float32:

    resblock     y = [W_1x1 | W_sc] . [lrelu(h); x] + (b_1x1 + b_sc),  h = conv_k3_dil_d(reflect_d(lrelu(x))) + b_d
    resstack     the blocks one after the other
    ct_resstack  LeakyReLU + ConvTranspose1d(k = 4, stride 2, padding 1), then the blocks
    out_bands    tanh(conv_k7(reflect_3(lrelu(x))))
    out_pqmf     out_bands, then PQMF synthesis (zero-stuff by N, scale by N, conv with G, padding taps / 2)

Rows are dense arrays (channels, positions); every function takes one row or a list of rows (a batch, run
as one sum over all its positions) and returns (result, largest |operand|) in the same form. The largest
operand is the maximum over what a split-f16 kernel has to split: x, every h, and every x_k that another
block consumes (not the final result); NaN if any of them holds one.

float32 is conv_np's term-by-term sum in the kernels' operand order (the second GEMM runs over
[lrelu(h); x] as one chain with the two biases added first), so its distance from float64 is the
tests' yardstick. float64 sums with a matrix product: the order of a float64 sum is far below what
that yardstick resolves. Pinned to torch and to oracle/melgan_np.py by tests/test_voc_oracle.py."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import conv_np as O


def _rows(x):
    return (list(x), True) if isinstance(x, (list, tuple)) else ([x], False)


def _absmax(rows):
    with np.errstate(invalid="ignore"):
        return max([float(np.abs(np.asarray(r, np.float64)).max()) if np.asarray(r).size else 0.0 for r in rows],
                   key=lambda v: (np.isnan(v), v))


def _worst(*vals):
    return max(vals, key=lambda v: (np.isnan(v), v))


def chain_sum32(w, g):
    """conv_np.chain_sum(w, g, np.float32) bit for bit (the same terms in the same order for every column),
    made quicker for the long rows of the persistent-loop tests: columns in blocks whose running sums stay
    in cache, no temporaries, blocks on a few threads (numpy releases the interpreter lock)."""
    Cout, Cin, K = w.shape
    w = np.ascontiguousarray(w, np.float32)
    acc = np.zeros((Cout, g.shape[2]), np.float32)

    def one(n):
        a = acc[:, n:n + 1024]
        t = np.empty(a.shape, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for ci in range(Cin):
                for k in range(K):
                    np.multiply(w[:, ci, k, None], g[ci, k, n:n + 1024][None, :], out=t)
                    a += t

    starts = range(0, g.shape[2], 1024)
    if len(starts) <= 1:
        for n in starts:
            one(n)
    else:
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
            list(ex.map(one, starts))
    return acc


def _gemm(w, g, dtype):
    """sum over (ci, tap) of w[co][ci][tap] g[ci][tap][n]: term by term in float32, a product in float64."""
    if dtype is np.float32:
        return chain_sum32(w, g)
    Cout = w.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        return w.reshape(Cout, -1).astype(dtype) @ g.reshape(-1, g.shape[2])


def _conv(xs, w, bias, dtype, dil=1, pad=0, pad_mode=0, act=0):
    """conv_np.conv_rows for one phase, through _gemm: rows xs -> rows (Cout, L_b)."""
    K = w.shape[2]
    lens = [x.shape[1] for x in xs]
    g = np.concatenate([O.gather_taps(x, n, K, dil, pad, pad_mode, 0, 0, 1, 1, act, dtype) for x, n in zip(xs, lens)], axis=2)
    with np.errstate(invalid="ignore", over="ignore"):
        z = _gemm(np.asarray(w), g, dtype) + np.asarray(bias).astype(dtype)[:, None]
    o = np.cumsum([0] + lens)
    return [z[:, o[i]:o[i + 1]] for i in range(len(xs))]


def _block(xs, wd, bd, w1, b1, ws, bs, dil, dtype):
    C = wd.shape[0]
    for x in xs:
        assert x.shape[1] > dil, "ReflectionPad1d(d) needs a row longer than d"
    xs = [np.asarray(x).astype(dtype) for x in xs]
    h = _conv(xs, wd, bd, dtype, dil=dil, pad=dil, pad_mode=1, act=1)
    wf = np.concatenate([np.asarray(w1).reshape(C, C), np.asarray(ws).reshape(C, C)], axis=1)[:, :, None]
    bf = np.asarray(b1).astype(dtype) + np.asarray(bs).astype(dtype)
    with np.errstate(invalid="ignore"):
        hx = [np.concatenate([O.lrelu(hh, dtype), x], axis=0) for hh, x in zip(h, xs)]
    y = _conv(hx, wf, bf, dtype)
    return y, _worst(_absmax(xs), _absmax(h))


def resblock(x, wd, bd, w1, b1, ws, bs, dil, dtype=np.float64):
    dtype = np.dtype(dtype).type
    xs, many = _rows(x)
    y, mx = _block(xs, wd, bd, w1, b1, ws, bs, dil, dtype)
    return (y if many else y[0]), mx


def _stack(xs, blocks, dtype):
    mx = 0.0
    for blk in blocks:
        xs, m = _block(xs, *blk, dtype)
        mx = _worst(mx, m)
    return xs, mx


def resstack(x, blocks, dtype=np.float64):
    """blocks: (wd, bd, w1, b1, ws, bs, dil) per block."""
    dtype = np.dtype(dtype).type
    xs, many = _rows(x)
    y, mx = _stack(xs, blocks, dtype)
    return (y if many else y[0]), mx


def conv_transpose2(x, ct_w, ct_b, dtype=np.float64):
    """LeakyReLU + ConvTranspose1d(k = 4, stride 2, padding 1) of one row or a list: (2C, L) -> (C, 2 L)."""
    dtype = np.dtype(dtype).type
    xs, many = _rows(x)
    with np.errstate(invalid="ignore", over="ignore"):
        y = [O.conv_transpose1d(r, np.asarray(ct_w), ct_b, 2, dtype, act=1) for r in xs]
    return y if many else y[0]


def ct_resstack(xin, ct_w, ct_b, blocks, dtype=np.float64):
    dtype = np.dtype(dtype).type
    xs, many = _rows(xin)
    x0 = conv_transpose2(xs, ct_w, ct_b, dtype)
    y, mx = _stack(x0, blocks, dtype)
    return (y if many else y[0]), _worst(mx, _absmax(xs))


def out_bands(x, wo, bo, dtype=np.float64):
    """LeakyReLU, ReflectionPad1d(3), Conv1d(k7), tanh: (C, L) -> (N, L)."""
    dtype = np.dtype(dtype).type
    xs, many = _rows(x)
    for r in xs:
        assert r.shape[1] > 3, "ReflectionPad1d(3) needs a row longer than 3"
    z = [np.tanh(v) for v in _conv([np.asarray(r).astype(dtype) for r in xs], np.asarray(wo), bo, dtype, pad=3, pad_mode=1, act=1)]
    return (z if many else z[0]), _absmax(xs)


def pqmf_synthesis(bands, G, dtype=np.float64):
    """oracle/melgan_np.pqmf_synthesis in dtype: bands (N, L), G (N, taps + 1) -> (1, N L)."""
    dtype = np.dtype(dtype).type
    N, L = bands.shape
    G = np.asarray(G).reshape(N, -1)
    u = np.zeros((N, N * L), dtype)
    u[:, ::N] = np.asarray(bands).astype(dtype) * dtype(N)
    return _conv([u], G[None], np.zeros(1), dtype, pad=(G.shape[1] - 1) // 2)[0]


def out_pqmf(x, wo, bo, G, dtype=np.float64):
    dtype = np.dtype(dtype).type
    xs, many = _rows(x)
    bands, mx = out_bands(xs, wo, bo, dtype)
    y = [pqmf_synthesis(b, G, dtype) for b in bands]
    return (y if many else y[0]), mx
