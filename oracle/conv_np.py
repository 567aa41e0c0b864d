"""The generic conv of tts_amd/csrc/common.h (ConvArgs) in plain numpy, at float64 or float32.

    out[b][co][q * out_mul + ph] = epi( bias[co] + sum_{ci, tap} W[ph][co][ci][tap] *
                                        in_act(src[b][ci][pad_map(q + tap * dil - pad_left[ph])]) )

for q in [0, Lq), Lq = (lens[b] + len_add) * q_mul, over an input of Lin = (lens[b] + len_add) * in_mul
positions. Rows are dense arrays here (channels, positions); memory layouts are the caller's business.
The sum is taken term by term in (ci, tap) order in the working dtype, so `dtype=np.float32` is a plain
float32 evaluation of the same expression: its distance from the float64 result is the yardstick the
GPU tests scale their tolerance by. The loops run over (ci, tap) and rows, never over positions.

Also: ConvTranspose1d(k = 2u, stride u, padding u / 2) by its definition, and its two descriptions as
generic convs (u polyphase 2-tap convs; one phase-merged GEMM), pinned to torch by
tests/test_conv_oracle.py."""
import numpy as np


def pad_index(i, L, mode):
    """Padded position i -> (position in [0, L), valid). mode 0 zero (valid = False outside), 1 reflect
    (edge not repeated, then clamped), 2 clamp."""
    i = np.asarray(i)
    inside = (i >= 0) & (i < L)
    if mode == 0:
        return np.where(inside, i, 0), inside
    j = i
    if mode == 1:
        j = np.where(j < 0, -j, j)
        j = np.where(j >= L, 2 * (L - 1) - j, j)
    j = np.clip(j, 0, L - 1)
    return np.where(inside, i, j), np.ones(i.shape, bool)


def lrelu(x, dtype):
    return np.where(x >= 0, x, dtype(0.2) * x)


def gather_taps(x, base_len, K, dil, pad_left, pad_mode, rep_pad, len_add, in_mul, q_mul, act, dtype):
    """One row x (Cin, Lsrc) -> the staged operand (Cin, K, Lq): in_act(src[pad_map(..)]), zeros where
    zero padding applies. Lsrc = Lin, or the raw lens[b] under rep_pad (virtual replicate padding of
    the raw source by rep_pad on each side; Lin counts the padded positions)."""
    base = base_len + len_add
    Lin, Lq = base * in_mul, base * q_mul
    i = np.arange(Lq)[None, :] + np.arange(K)[:, None] * dil - pad_left
    idx, valid = pad_index(i, Lin, pad_mode)
    Lsrc = base_len if rep_pad else Lin
    if rep_pad:
        idx = idx - rep_pad
    idx = np.clip(idx, 0, Lsrc - 1)
    xs = np.asarray(x)[:, :Lsrc].astype(dtype)
    if act:
        xs = lrelu(xs, dtype)
    return np.where(valid[None], xs[:, idx], dtype(0))


def chain_sum(w, g, dtype):
    """sum_{ci, tap} w[co][ci][tap] * g[ci][tap][n], one term after the other in dtype."""
    Cout, Cin, K = w.shape
    wd = w.astype(dtype)
    acc = np.zeros((Cout, g.shape[2]), dtype)
    for ci in range(Cin):
        for k in range(K):
            acc += wd[:, ci, k, None] * g[ci, k][None, :]
    return acc


def sigmoid(x, dtype):
    return dtype(1) / (dtype(1) + np.exp(-x))


def epilogue(z, epi, dtype, resid=None, resid_rows=0, aux=None):
    """z (Cout, T) = conv + bias. Forms (conv_epi.h): 0 none, 1 relu, 2 tanh, each followed by the
    residual on rows < resid_rows (0: all rows); 3 gate tanh(u) sigmoid(g) over row pairs (u, g) =
    (2c, 2c + 1), aux (Cout,) added first when given; 4 coupling reverse (resid[c] - u) exp(-g);
    5 coupling reverse on the second half of resid's channels, then the inverse InvConvNear (4 x 4 over
    {x0[2m], x0[2m + 1], x1[2m], x1[2m + 1]}) and ActNorm from aux (Cout, 6) = {w[4], bias, scale};
    6 GLU u sigmoid(g)."""
    z = z.astype(dtype)
    if epi in (0, 1, 2):
        v = z if epi == 0 else (np.maximum(z, dtype(0)) if epi == 1 else np.tanh(z))
        if resid is not None:
            rows = resid_rows if resid_rows > 0 else z.shape[0]
            v = v.copy()
            v[:rows] += np.asarray(resid).astype(dtype)[:rows]
        return v
    u, g = z[0::2], z[1::2]
    if epi == 3:
        if aux is not None:
            a = np.asarray(aux).astype(dtype)
            u, g = u + a[0::2, None], g + a[1::2, None]
        return np.tanh(u) * sigmoid(g, dtype)
    if epi == 6:
        return u * sigmoid(g, dtype)
    x = np.asarray(resid).astype(dtype)
    if epi == 4:
        return (x - u) * np.exp(-g)
    assert epi == 5 and z.shape[0] % 4 == 0
    Ch = z.shape[0] // 2
    a = np.asarray(aux).astype(dtype)
    x1 = (x[Ch:] - u) * np.exp(-g)  # channel Ch + c from rows (2c, 2c + 1)
    out = np.empty_like(x)
    for m in range(0, Ch, 2):
        grp = [x[m], x[m + 1], x1[m], x1[m + 1]]
        for c in (m, m + 1, Ch + m, Ch + m + 1):
            v = a[c, 0] * grp[0]
            for k in (1, 2, 3):
                v = v + a[c, k] * grp[k]
            out[c] = (v - a[c, 4]) * a[c, 5]
    return out


def conv_rows(xs, w, bias, lens, dtype=np.float64, dil=1, pad_left=(0,), pad_mode=0, rep_pad=0, len_add=0, in_mul=1,
              q_mul=1, out_mul=1, act=0, epi=0, resid=None, resid_rows=0, aux=None):
    """The whole call on a batch: xs[b] (Cin, Lsrc_b), w (Cout, Cin, K) or (nphase, Cout, Cin, K), lens[b]
    -> list of (rows, Lq_b * out_mul) arrays (rows = Cout, or Cout / 2 for the pair forms 3, 4, 6).
    resid[b]: the residual row, shaped like the output (forms 0-2, 4) or (Cout, T) (form 5);
    aux: per-row (B, Cout) for form 3, the (Cout, 6) table for form 5. out_mul == nphase."""
    dtype = np.dtype(dtype).type
    w = np.asarray(w)
    if w.ndim == 3:
        w = w[None]
    nphase, Cout, Cin, K = w.shape
    assert out_mul == nphase and len(pad_left) >= nphase
    Lq = [(int(n) + len_add) * q_mul for n in lens]
    z = [np.empty((Cout, n * out_mul), dtype) for n in Lq]
    b_ = np.asarray(bias).astype(dtype)[:, None]
    for ph in range(nphase):
        g = np.concatenate([gather_taps(x, int(n), K, dil, pad_left[ph], pad_mode, rep_pad, len_add, in_mul, q_mul,
                                        act, dtype) for x, n in zip(xs, lens)], axis=2)
        acc = chain_sum(w[ph], g, dtype) + b_
        o = 0
        for r, n in enumerate(Lq):
            z[r][:, ph::out_mul] = acc[:, o:o + n]
            o += n
    out = []
    for r in range(len(xs)):
        a = None if aux is None else (aux[r] if epi == 3 else aux)
        out.append(epilogue(z[r], epi, dtype, None if resid is None else resid[r], resid_rows, a))
    return out


# ---- ConvTranspose1d(k = 2u, stride u, padding u / 2) ----
def conv_transpose1d(x, wt, bias, u, dtype=np.float64, act=0):
    """By definition: out[co][i u - u / 2 + k] += x[ci][i] wt[ci][co][k]; x (Cin, L) -> (Cout, L u)."""
    dtype = np.dtype(dtype).type
    Cin, Cout, K = wt.shape
    assert K == 2 * u
    xs = np.asarray(x).astype(dtype)
    if act:
        xs = lrelu(xs, dtype)
    L, p = xs.shape[1], u // 2
    wd = wt.astype(dtype)
    buf = np.zeros((Cout, (L + 1) * u), dtype)  # output position t at column t + p
    for ci in range(Cin):
        for k in range(K):
            buf[:, k:k + L * u:u] += wd[ci, :, k, None] * xs[ci][None, :]
    return buf[:, p:p + L * u] + np.asarray(bias).astype(dtype)[:, None]


def convT_polyphase(wt, u):
    """The polyphase description: phase ph is a 2-tap conv Wm[ph] (Cout, Cin, 2) with pad_left[ph], its
    output position q lands at q u + ph. Input q + delta, delta = dmin + tap, meets kernel tap
    k = ph + u / 2 - delta u."""
    Cin, Cout, K = wt.shape
    p = u // 2
    Wm = np.zeros((u, Cout, Cin, 2), wt.dtype)
    pls = []
    for ph in range(u):
        dmin = (ph + p) // u - 1
        pls.append(-dmin)
        for jj in range(2):
            Wm[ph, :, :, jj] = wt[:, :, ph + p - (dmin + jj) * u].T
    return Wm, pls


def convT_merged(x, wt, bias, u, dtype=np.float64, act=0):
    """The phase-merged description (ConvArgs::merged_u): one 2-tap conv with rows m = co u + ph over
    inputs q - 1 and q (zero padded) for q in [0, L]; phases >= u / 2 write output position
    (q - 1) u + ph, the others q u + ph."""
    dtype = np.dtype(dtype).type
    Cin, Cout, _ = wt.shape
    Wm, _ = convT_polyphase(wt, u)
    W = Wm.transpose(1, 0, 2, 3).reshape(Cout * u, Cin, 2)
    L = np.asarray(x).shape[1]
    xe = np.concatenate([np.asarray(x), np.zeros((Cin, 1), np.asarray(x).dtype)], axis=1)  # input L is zero padding
    g = gather_taps(xe, L + 1, 2, 1, 1, 0, 0, 0, 1, 1, act, dtype)
    z = chain_sum(W, g, dtype) + np.repeat(np.asarray(bias).astype(dtype), u)[:, None]
    out = np.empty((Cout, L * u), dtype)
    for ph in range(u):
        hi = 1 if 2 * ph >= u else 0
        out[:, ph::u] = z[ph::u, hi:hi + L]
    return out
