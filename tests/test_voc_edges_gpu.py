"""The vocoder's own kernels (resblock.hip fp32, resblock_x3.hip, resstack_x3.hip with and without the fused
ConvTranspose, melgan_out.hip) one launch at a time through tts_test_voc (the loaders' packing, the launchers
called directly), against oracle/voc_np.py in float64 (pinned to torch by tests/test_voc_oracle.py): tile and
halo edges, ragged and widest batches, the persistent loop with more tiles than twice the CUs, upper-bound
host lengths, store forms, refusals and the range flag.

Harness of test_conv_edges_gpu.py: every source is NaN past each row's length, between rows and in a margin;
every output buffer carries a sentinel in each element the call must not write (past a row's positions,
between rows, in a margin on both sides); both are checked on every call.

Tolerance: per case e32 = max |oracle(float32) - oracle(float64)| of the same chained
operation; every output element is within 8 x e32 of the float64 oracle (output kernels: 8 x max(e32, one
float32 spacing at the output scale 1)); the split-f16 kernels are also within 2 x the fp32 block kernel's
error on the same case + 2e-6 x max(1, max |ref|). Each comparison prints error, e32 and ratio first.
Weights are N(0, 1) / sqrt(fan-in), biases N(0, 0.5), inputs N(0, 1) unless a case says otherwise.

TQ is what the hook reports (one probe launch per kernel); the tables below only name the template
instantiation each case is expected to run."""
import numpy as np
import pytest
import torch

from oracle import voc_np as V

pytestmark = pytest.mark.gpu

SENT = np.float32(-12345.678)
MARGIN = 64  # sentinel / NaN elements on both sides of a buffer (a multiple of 4: keeps the alignment)
GAP = 8      # elements between two rows of a batch (a multiple of 4)
F16_MAX = 65504.0
CHANNELS = [32, 48, 64, 96, 128, 192, 256]
DILS = [1, 3, 9, 27]
# the instantiations of launch_resblock / launch_resblock_x3 / launch_resstack_x3 by channel count
TQ_RB = {192: 32, 96: 64, 48: 128, 256: 32, 128: 64, 64: 128, 32: 64}       # resblock_kernel<C, TQ, ..>
TQ_RBX3 = {192: 64, 96: 128, 48: 192, 256: 32, 128: 64, 64: 128, 32: 192}   # resblock_x3_kernel<C, TQ, ..>
TQ_RSX3 = {48: 208, 96: 96}                                                  # resstack_x3_kernel<C, TQ, .., CTU = 0>
TQ_CT = 208                                                                  # resstack_x3_kernel<48, 208, 4, 4, 2>
TQ_PQMF, TQ_OUT1 = 1008, 4096                                                # out_pqmf_kernel<C>, out_conv1_kernel
_cache = {}
ratios = {}  # kind -> largest err / e32 seen (printed with every comparison)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


def _engine():
    from tts_amd._lib import get_engine
    return get_engine(_dev())


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _up4(n):
    return (n + 3) // 4 * 4


# ---- weights and inputs ----
def _blocks(C, dils, seed=0):
    rs = np.random.RandomState(1000 * seed + C)
    n = lambda s, shape: rs.normal(0, s, shape).astype(np.float32)
    return [(n(1 / np.sqrt(3 * C), (C, C, 3)), n(0.5, C), n(1 / np.sqrt(C), (C, C, 1)), n(0.5, C),
             n(1 / np.sqrt(C), (C, C, 1)), n(0.5, C), int(d)) for d in dils]


def _ct(C=48, seed=0):
    rs = np.random.RandomState(77 + seed)
    return rs.normal(0, 1 / np.sqrt(4 * C), (2 * C, C, 4)).astype(np.float32), rs.normal(0, 0.5, C).astype(np.float32)


def _outw(C, N, seed=0):
    rs = np.random.RandomState(55 + seed + C)
    return rs.normal(0, 1 / np.sqrt(7 * C), (N, C, 7)).astype(np.float32), rs.normal(0, 0.5, N).astype(np.float32)


def _G():
    from tts_amd.pqmf import pqmf_filters
    return np.ascontiguousarray(np.asarray(pqmf_filters()[1], np.float32).reshape(4, -1))


def _xrows(C, lens, seed=0):
    rs = np.random.RandomState(31 * seed + C + 7 * len(lens) + int(lens[0]))
    return [rs.normal(0, 1, (C, int(n))).astype(np.float32) for n in lens]


# ---- one launch ----
def _layout(C, L, extra=0):
    """(batch stride, channel stride, elements) of a (B, C, L_b) tensor: rows one after the other, channel
    stride = the longest row + 3 up to a multiple of 4 (+ extra), GAP spare elements per row. Where the last
    row is far longer than the others (the persistent-loop batches) the rows lie side by side inside one
    channel stride instead, batch stride = the longest short row: a few MB where B whole rows would be a GB."""
    B = len(L)
    if B >= 2 and L[-1] > 8 * max(L[:-1]):
        sb = _up4(max(L[:-1]) + 3) + GAP
        sc = (B - 1) * sb + _up4(L[-1] + 3) + GAP + extra
        return sb, sc, C * sc
    sc = _up4(max(L) + 3) + extra
    return C * sc + GAP, sc, B * (C * sc + GAP)


def _flat(rows, sb, sc, n):
    """rows[b] (C, T_b) -> (device buffer that is NaN wherever it is not a row's data, row 0's address, host copy)."""
    a = np.full(2 * MARGIN + n, np.nan, np.float32)
    for b, r in enumerate(rows):
        C, T = r.shape
        idx = MARGIN + b * sb + np.arange(C)[:, None] * sc + np.arange(T)[None, :]
        a[idx] = r
    t = torch.from_numpy(a).to(_dev())
    return t, t.data_ptr() + 4 * MARGIN, a


def _unchanged(t, a):
    return np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))


def run(kind, C, rows, blocks=(), ct=None, out=None, G=None, bounds=None, mul=1, ls_extra=0, y_off=0, x_extra=0, yb_extra=0,
        max_q=None):
    """One tts_test_voc call on rows[b] (Cx, Lin_b) -> (output rows as numpy, tq, flag). Checks the sentinels.
    kinds 0-2 share one stride pair between x and y (Ls = the longest row + 3, up to a multiple of 4, + ls_extra);
    kind 3 reads (2C, Lin) rows and writes (C, 2 Lin); kind 4 writes 4 max_q samples per row; y_off shifts
    the output by floats."""
    B = len(rows)
    Lin = [r.shape[1] for r in rows]
    L = [2 * n for n in Lin] if kind == 3 else Lin   # positions the kernel's tiles run over
    assert all(n % mul == 0 for n in L)
    lens = [n // mul for n in L]
    mq = max(L) if max_q is None else max_q
    if kind <= 3:
        ys, yrows, ylen = _layout(C, L, ls_extra), C, L
        xs_ = _layout(2 * C, Lin) if kind == 3 else ys
    else:
        xs_ = _layout(C, L, x_extra)
        yrows = 1
        ylen = [4 * mq] * B if kind == 4 else L
        yb = _up4(max(ylen) + 3) + GAP + yb_extra
        ys = (yb, 0, B * yb)
    xt, xp, xh = _flat(rows, *xs_)
    yflat = np.full(2 * MARGIN + y_off + ys[2], SENT, np.float32)
    written = np.zeros(yflat.shape, bool)
    idx = []
    for b in range(B):
        i = MARGIN + y_off + b * ys[0] + np.arange(yrows)[:, None] * ys[1] + np.arange(ylen[b])[None, :]
        idx.append(i)
        written[i] = True
    if kind == 4:  # the kernel writes all of [0, 4 max_q): no NaN may survive there
        yflat[written] = np.nan
    yt = torch.from_numpy(yflat).to(_dev())
    tq, flag = _engine().voc_test(kind, C, lens, (xp, xs_[:2]), (yt.data_ptr() + 4 * (MARGIN + y_off), ys[:2]), mq, _dev(),
                                  blocks=blocks, ct=ct, out=out, G=G, bounds=bounds, mul=mul)
    h = yt.cpu().numpy()
    assert (h[~written].view(np.uint32) == SENT.view(np.uint32)).all(), "the call wrote outside its result"
    assert _unchanged(xt, xh), "the call wrote into its source"
    return [h[i] for i in idx], tq, flag


def _tq(kind, C):
    """The tile width the hook reports for this kernel, from one small launch."""
    key = ("tq", kind, C)
    if key not in _cache:
        if kind <= 3:
            d = (1, 1, 1) if kind >= 2 else (1,)
            rows = _xrows(2 * C if kind == 3 else C, (20,))
            _cache[key] = run(kind, C, rows, blocks=_blocks(C, d), ct=_ct() if kind == 3 else None, mul=2 if kind == 3 else 1)[1]
        elif kind == 4:
            _cache[key] = run(4, C, _xrows(C, (8,)), out=_outw(C, 4), G=_G())[1]
        else:
            _cache[key] = run(5, C, _xrows(C, (8,)), out=_outw(C, 1))[1]
    return _cache[key]


# ---- oracle, once per case ----
def _oracle(key, fn):
    """fn(dtype) -> (rows, largest operand); cached: (float64 rows, per-row e32, largest operand)."""
    if key not in _cache:
        r64, mx = fn(np.float64)
        r32, _ = fn(np.float32)
        with np.errstate(invalid="ignore"):
            e32 = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32, r64)]
        for r in r64:
            r.setflags(write=False)
        _cache[key] = (r64, e32, mx)
    return _cache[key]


def _err(o, r):
    return float(np.abs(o.astype(np.float64) - r).max())


def within(what, kind, outs, ref, e32, k32=None, floor=0.0):
    """Every row within 8 x e32 of the float64 oracle; with k32 (the fp32 block kernel's error per row) also
    within 2 x k32 + 2e-6 x max(1, max |ref|). Returns the per-row errors."""
    errs = []
    for b, (o, r) in enumerate(zip(outs, ref)):
        assert np.isfinite(o).all(), f"{what} row {b}: non-finite output"
        k, e = _err(o, r), max(e32[b], floor)
        ratio = k / max(e, 1e-30)
        ratios[kind] = max(ratios.get(kind, 0.0), ratio)
        extra = "" if k32 is None else f" fp32 kernel {k32[b]:.3e}"
        print(f"{what} row {b} L {r.shape[1]}: kind {kind} err {k:.3e} e32 {e:.3e} ratio {ratio:.2f}{extra}")
        assert k <= 8 * e, f"{what} row {b}: kind {kind} error {k:.3e} > 8 x {e:.3e}"
        if k32 is not None:
            scale = max(1.0, float(np.abs(r).max()))
            assert k <= 2 * k32[b] + 2e-6 * scale, f"{what} row {b}: split-f16 {k:.3e} vs fp32 kernel {k32[b]:.3e}"
        errs.append(k)
    return errs


def _same(what, a, b):
    for i, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), f"{what}: row {i} differs bit for bit"


def _raises(text, *a, **kw):
    with pytest.raises(RuntimeError) as ei:
        run(*a, **kw)
    assert text in str(ei.value), str(ei.value)


# =====================================================================================================
# Block kernels: kind 0 (fp32) and kind 1 (split-f16)
# =====================================================================================================
def block_case(what, C, d, rows, seed=0, x3_kw=None, want_flag=0):
    """Both block kernels on one batch against the oracle; returns (kind 1 rows, its tile width)."""
    blk = _blocks(C, (d,), seed)
    key = ("rb", C, d, seed, tuple(r.shape[1] for r in rows), float(rows[0][0, 0]))
    ref, e32, mx = _oracle(key, lambda dt: V.resblock(rows, *blk[0], dt))
    assert mx < F16_MAX / 4, f"{what}: the oracle's largest operand {mx} is not clearly inside the f16 range"
    o32, tq32, f32 = run(0, C, rows, blocks=blk)
    o16, tq16, f16 = run(1, C, rows, blocks=blk, **(x3_kw or {}))
    assert tq32 == TQ_RB[C] and f32 == 0, f"{what}: resblock_kernel<{C}> reports tq {tq32}, flag {f32}"
    assert tq16 == TQ_RBX3[C], f"{what}: resblock_x3_kernel<{C}> reports tq {tq16}"
    assert f16 == want_flag, f"{what}: range flag {f16}"
    k32 = within(what, 0, o32, ref, e32)
    within(what, 1, o16, ref, e32, k32)
    return o16, tq16


@pytest.mark.parametrize("C", CHANNELS)
def test_block_single_rows_at_tile_and_reflection_edges(C):
    """L = d + 1 (the shortest row ReflectionPad1d(d) takes), TQ - 1, TQ, TQ + 1, TQ + d, 2 TQ + 1 of either
    kernel's tile, each as its own B = 1 call, every dilation."""
    tqs = sorted({_tq(0, C), _tq(1, C)})
    for d in DILS:
        lens = sorted({d + 1} | {n for tq in tqs for n in (tq - 1, tq, tq + 1, tq + d, 2 * tq + 1) if n > d})
        for L in lens:
            block_case(f"C {C} d {d}", C, d, _xrows(C, (L,), seed=d))


@pytest.mark.parametrize("C", CHANNELS)
def test_block_ragged_batch_rows_equal_their_single_calls(C):
    """B = 3 with lengths (2 TQ + 1, d + 1, TQ): each row bit-identical to its own B = 1 call."""
    tq = _tq(1, C)
    for d in DILS:
        rows = _xrows(C, (2 * tq + 1, d + 1, tq), seed=d)
        blk = _blocks(C, (d,))
        o16, _ = block_case(f"ragged C {C} d {d}", C, d, rows)
        o32 = run(0, C, rows, blocks=blk)[0]
        for b, r in enumerate(rows):
            _same(f"C {C} d {d} kind 1 row {b} vs B = 1", [o16[b]], run(1, C, [r], blocks=blk)[0])
            _same(f"C {C} d {d} kind 0 row {b} vs B = 1", [o32[b]], run(0, C, [r], blocks=blk)[0])


@pytest.mark.parametrize("C", CHANNELS)
def test_block_widest_batch(C):
    """B = 64, lengths d + 1 .. d + 64: all 64 lanes of the tile scan hold a row. Rows equal their B = 1 calls
    bit for bit (every fourth row is run alone: 16 single calls per kernel); B = 65 is the launcher's error."""
    for d in (1, 27):
        rows = _xrows(C, [d + 1 + i for i in range(64)], seed=d)
        blk = _blocks(C, (d,))
        o16, _ = block_case(f"B 64 C {C} d {d}", C, d, rows)
        o32 = run(0, C, rows, blocks=blk)[0]
        for b in range(0, 64, 4):
            _same(f"C {C} d {d} kind 1 row {b} vs B = 1", [o16[b]], run(1, C, [rows[b]], blocks=blk)[0])
            _same(f"C {C} d {d} kind 0 row {b} vs B = 1", [o32[b]], run(0, C, [rows[b]], blocks=blk)[0])
    _raises("at most 64 utterances", 1, C, _xrows(C, [30] * 65), blocks=_blocks(C, (1,)))


@pytest.mark.parametrize("C", CHANNELS)
def test_block_x3_per_position_stores_equal_vector_stores(C):
    """Ls % 4 != 0 and an output one float off 16-byte alignment take the per-position stores (vec = false)."""
    tq = _tq(1, C)
    for d in (1, 9):
        rows = _xrows(C, (tq + 5, d + 1, 2 * tq - 3), seed=d)
        blk = _blocks(C, (d,))
        o16, _ = block_case(f"aligned C {C} d {d}", C, d, rows)
        for what, kw in (("Ls % 4 == 1", dict(ls_extra=1)), ("Ls % 4 == 2", dict(ls_extra=2)), ("y + 1 float", dict(y_off=1))):
            alt, tq2, flag = run(1, C, rows, blocks=blk, **kw)
            assert tq2 == tq and flag == 0
            _same(f"C {C} d {d} {what} vs aligned", alt, o16)


def _persistent_lens(tq, lo, step=1):
    """2 n + 1 tiles of tq (n = CUs) in B = 64 rows (the widest batch the kernels take): 63 short rows of
    1, 2, 3, 1, .. tiles, every second one with a last tile of `step` positions (where the row stays >= lo),
    then the long row with the remainder, its last tile `step` wide too. With grid n the first workgroups'
    tiles i, i + n lie in a short row and the long row; workgroup 0 takes a third tile."""
    n = _ncu()
    short = []
    for i in range(63):
        t = 1 + i % 3
        L = (t - 1) * tq + (step if i % 2 == 0 else tq - 4 * (i % 5))
        short.append(max(L, lo + (i % 2) * step))
    tiles = sum(-(-L // tq) for L in short)
    long_t = 2 * n + 1 - tiles
    assert long_t >= 1
    lens = short + [long_t * tq - (tq - step)]
    assert sum(-(-L // tq) for L in lens) == 2 * n + 1 and len(lens) == 64
    return lens


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("d", [1, 27])
def test_block_x3_persistent_loop(C, d):
    """More tiles than twice the CUs: the prefetch of the next tile, the weight ring running on into it, the
    EARLY register-set parity (NSC = 1 at C = 32, 2 at 48 / 64, odd at 96, even > 2 at 128 / 192 / 256) and
    the barriers between tiles."""
    tq = _tq(1, C)
    lens = _persistent_lens(tq, d + 1)
    assert sum(1 for L in lens if L % tq == 1) >= 3  # last tiles of one position
    block_case(f"persistent C {C} d {d} ({2 * _ncu() + 1} tiles)", C, d, _xrows(C, lens, seed=d))


@pytest.mark.parametrize("C", CHANNELS)
def test_block_x3_upper_bound_host_lengths(C):
    """h_bounds = true length + (0, 1, TQ, 3 TQ): the grid comes from the bounds (here larger than the tile
    count the kernel arrives at from the device lengths), the output from the true lengths."""
    tq = _tq(1, C)
    d = 3
    lens = (tq + 1, d + 1, 2 * tq, tq - 1)
    rows = _xrows(C, lens)
    blk = _blocks(C, (d,))
    o16, _ = block_case(f"bounds C {C}", C, d, rows)
    bounds = [n + a for n, a in zip(lens, (0, 1, tq, 3 * tq))]
    assert sum(-(-n // tq) for n in bounds) > sum(-(-n // tq) for n in lens) and sum(-(-n // tq) for n in bounds) <= _ncu()
    alt, tq2, flag = run(1, C, rows, blocks=blk, bounds=bounds)
    assert tq2 == tq and flag == 0
    _same(f"C {C} bounds vs exact lengths", alt, o16)


def test_block_refusals():
    _raises("unsupported channel count", 0, 80, _xrows(80, (30,)), blocks=_blocks(80, (1,)))
    with pytest.raises(RuntimeError):  # no split weights exist for it: the launcher's own check
        run(1, 80, _xrows(80, (30,)), blocks=_blocks(80, (1,)))
    _raises("dilation must be in [1, 27]", 1, 48, _xrows(48, (40,)), blocks=_blocks(48, (28,)))
    _raises("dilation must be in [1, 27]", 0, 48, _xrows(48, (40,)), blocks=_blocks(48, (28,)))


# =====================================================================================================
# Stack kernel: kind 2
# =====================================================================================================
STACK_DILS = [(1, 3, 9), (9, 3, 1), (1, 1, 1), (14, 1, 1)]


def _fp32_chain(C, rows, blocks):
    for blk in blocks:
        rows = run(0, C, rows, blocks=[blk])[0]
    return rows


def stack_case(what, C, dils, rows, seed=0, **kw):
    """kind 2 on a batch, three kind-1 launches and three kind-0 launches on the same data, one oracle."""
    blocks = _blocks(C, dils, seed)
    key = ("rs", C, dils, seed, tuple(r.shape[1] for r in rows), float(rows[0][0, 0]))
    ref, e32, mx = _oracle(key, lambda dt: V.resstack(rows, blocks, dt))
    assert mx < F16_MAX / 4, f"{what}: the oracle's largest operand {mx} is not clearly inside the f16 range"
    k32 = [_err(o, r) for o, r in zip(_fp32_chain(C, rows, blocks), ref)]
    o2, tq, flag = run(2, C, rows, blocks=blocks, **kw)
    assert tq == TQ_RSX3[C] and flag == 0, f"{what}: resstack_x3_kernel<{C}> reports tq {tq}, flag {flag}"
    within(what, 2, o2, ref, e32, k32)
    o1 = rows
    for blk in blocks:
        o1, _, f1 = run(1, C, o1, blocks=[blk])
        assert f1 == 0
    within(what + " (three kind-1 launches)", 1, o1, ref, e32, k32)
    return o2, tq


@pytest.mark.parametrize("C", [48, 96])
@pytest.mark.parametrize("dils", STACK_DILS)
def test_stack_single_rows(C, dils):
    """L = 17 (the shortest row resstack_x3_fits admits), 18, 32, TQ - 1, TQ, TQ + 1, TQ + 12, 2 TQ + 1."""
    tq = _tq(2, C)
    for L in (17, 18, 32, tq - 1, tq, tq + 1, tq + 12, 2 * tq + 1):
        stack_case(f"stack C {C} dils {dils}", C, dils, _xrows(C, (L,), seed=sum(dils)))


@pytest.mark.parametrize("C", [48, 96])
def test_stack_batches_rows_equal_their_single_calls(C):
    tq = _tq(2, C)
    dils = (1, 3, 9)
    blocks = _blocks(C, dils)
    rows = _xrows(C, (2 * tq + 1, 17, tq), seed=1)
    o2, _ = stack_case(f"stack ragged C {C}", C, dils, rows)
    for b, r in enumerate(rows):
        _same(f"stack C {C} row {b} vs B = 1", [o2[b]], run(2, C, [r], blocks=blocks)[0])
    rows = _xrows(C, [17 + i for i in range(64)], seed=2)
    o2, _ = stack_case(f"stack B 64 C {C}", C, dils, rows)
    for b in range(0, 64, 4):
        _same(f"stack C {C} B 64 row {b} vs B = 1", [o2[b]], run(2, C, [rows[b]], blocks=blocks)[0])


@pytest.mark.parametrize("C", [48, 96])
def test_stack_persistent_loop(C):
    tq = _tq(2, C)
    lens = _persistent_lens(tq, 17)
    stack_case(f"stack persistent C {C} ({2 * _ncu() + 1} tiles)", C, (1, 3, 9), _xrows(C, lens, seed=3))


@pytest.mark.parametrize("C", [48, 96])
def test_stack_upper_bound_host_lengths(C):
    tq = _tq(2, C)
    lens = (tq + 1, 17, 2 * tq, tq - 1)
    rows = _xrows(C, lens, seed=4)
    o2, _ = stack_case(f"stack bounds C {C}", C, (1, 3, 9), rows)
    bounds = [n + a for n, a in zip(lens, (0, 1, tq, 3 * tq))]
    alt, tq2, flag = run(2, C, rows, blocks=_blocks(C, (1, 3, 9)), bounds=bounds)
    assert tq2 == tq and flag == 0
    _same(f"stack C {C} bounds vs exact lengths", alt, o2)


@pytest.mark.parametrize("C", [48, 96])
def test_stack_refusals(C):
    blocks = _blocks(C, (1, 3, 9))
    msg = "resstack_x3: unaligned rows, more than 64 utterances or an utterance shorter than the reflection pad"
    _raises(msg, 2, C, _xrows(C, (16,)), blocks=blocks)
    _raises(msg, 2, C, _xrows(C, (40,)), blocks=blocks, ls_extra=1)
    _raises(msg, 2, C, _xrows(C, (40,)), blocks=blocks, y_off=1)
    _raises(msg, 2, C, _xrows(C, [20] * 65), blocks=blocks)
    _raises("resstack_x3: shape not covered", 2, C, _xrows(C, (40,)), blocks=_blocks(C, (15, 1, 1)))
    _raises("resstack_x3: shape not covered", 2, 64, _xrows(64, (40,)), blocks=_blocks(64, (1, 3, 9)))


# =====================================================================================================
# Fused ConvTranspose + stack: kind 3 (C = 48 from 96 channels)
# =====================================================================================================
def _conv_transpose(rows, ct, merged):
    """LeakyReLU + ConvTranspose1d(u = 2) through tts_test_conv: the phase-merged split-f16 form (merged_u = 2)
    or the two polyphase convs on the fp32 kernel. rows (2C, Lin_b) -> rows (C, 2 Lin_b)."""
    C, Lin = ct[0].shape[1], [r.shape[1] for r in rows]
    xs_, ys = _layout(2 * C, Lin), _layout(C, [2 * n for n in Lin])
    xt, xp, xh = _flat(rows, *xs_)
    y = torch.full((2 * MARGIN + ys[2],), float(SENT), dtype=torch.float32, device=_dev())
    eng = _engine()
    eng.set_gemm_mode("x3" if merged else "f32")
    try:
        info = eng.conv_test(ct[0], ct[1], Lin, (xp, (xs_[0], xs_[1], 1), 2 * C, 1), (y.data_ptr() + 4 * MARGIN, (ys[0], ys[1], 1)),
                             max(Lin) + (1 if merged else 0), _dev(), transposed=True, nphase=2, out_mul=1 if merged else 2,
                             merged_u=2 if merged else 0)
    finally:
        eng.set_gemm_mode("x3")
    assert info[0] == merged and info[2] == 0
    h = y.cpu().numpy()
    return [h[MARGIN + b * ys[0] + np.arange(C)[:, None] * ys[1] + np.arange(2 * n)[None, :]] for b, n in enumerate(Lin)]


def _two_launches(rows, ct, blocks, mul=2, bounds=None):
    """The merged ConvTranspose through tts_test_conv (merged_u = 2), its output through kind 2."""
    return run(2, 48, _conv_transpose(rows, ct, True), blocks=blocks, mul=mul, bounds=bounds)[0]


def ct_case(what, rows, dils=(1, 3, 9), seed=0, mul=2, bounds=None):
    C = 48
    blocks, ct = _blocks(C, dils, seed), _ct(C, seed)
    key = ("ct", dils, seed, tuple(r.shape[1] for r in rows), float(rows[0][0, 0]))
    ref, e32, mx = _oracle(key, lambda dt: V.ct_resstack(rows, ct[0], ct[1], blocks, dt))
    assert mx < F16_MAX / 4, f"{what}: the oracle's largest operand {mx} is not clearly inside the f16 range"
    # the fp32 kernels on the same case: the polyphase ConvTranspose (conv.hip), then three kind-0 launches
    k32 = [_err(o, r) for o, r in zip(_fp32_chain(C, _conv_transpose(rows, ct, False), blocks), ref)]
    o3, tq, flag = run(3, C, rows, blocks=blocks, ct=ct, mul=mul, bounds=bounds)
    assert tq == TQ_CT and flag == 0, f"{what}: resstack_x3_kernel<48, .., CTU = 2> reports tq {tq}, flag {flag}"
    within(what, 3, o3, ref, e32, k32)
    _same(f"{what}: kind 3 vs merged ConvTranspose + kind 2", o3, _two_launches(rows, ct, blocks, mul, bounds))
    return o3, tq


def test_ct_single_rows():
    """Lin = 9, 10 (L = 18, 20: the shortest), 103, 104, 105 (a tile less a pair, one tile, a second tile of two
    positions), 208, 209 (two tiles, a third of two positions)."""
    assert _tq(3, 48) == TQ_CT
    for Lin in (9, 10, 103, 104, 105, 208, 209):
        ct_case(f"ct Lin {Lin}", _xrows(96, (Lin,), seed=Lin))


def test_ct_length_factor_64():
    """mul = 64 as the last MB-MelGAN stage runs (L = 64 frames, so Lin = 32 frames): one tile, a tile ending on
    a frame boundary short of TQ, two tiles, five."""
    for frames in (1, 3, 4, 16):
        ct_case(f"ct mul 64 frames {frames}", _xrows(96, (32 * frames,), seed=frames), mul=64)


def test_ct_batches_rows_equal_their_single_calls():
    blocks, ct = _blocks(48, (1, 3, 9)), _ct()
    rows = _xrows(96, (209, 9, 104), seed=5)
    o3, _ = ct_case("ct ragged", rows)
    for b, r in enumerate(rows):
        _same(f"ct row {b} vs B = 1", [o3[b]], run(3, 48, [r], blocks=blocks, ct=ct, mul=2)[0])
    rows = _xrows(96, [9 + i for i in range(64)], seed=6)
    o3, _ = ct_case("ct B 64", rows)
    for b in range(0, 64, 4):
        _same(f"ct B 64 row {b} vs B = 1", [o3[b]], run(3, 48, [rows[b]], blocks=blocks, ct=ct, mul=2)[0])


def test_ct_persistent_loop():
    lens = _persistent_lens(TQ_CT, 18, step=2)
    assert all(L % 2 == 0 for L in lens)
    ct_case(f"ct persistent ({2 * _ncu() + 1} tiles)", _xrows(96, [L // 2 for L in lens], seed=7))


def test_ct_upper_bound_host_lengths():
    tq = _tq(3, 48)
    Lin = (tq // 2 + 1, 9, tq, tq // 2 - 1)
    rows = _xrows(96, Lin, seed=8)
    o3, _ = ct_case("ct bounds", rows)
    bounds = [n + a for n, a in zip(Lin, (0, 1, tq // 2, 3 * tq // 2))]  # in the hook's units: L = 2 h_lens
    alt = ct_case("ct bounds, upper", rows, bounds=bounds)[0]
    _same("ct bounds vs exact lengths", alt, o3)


def test_ct_refusals():
    blocks, ct = _blocks(48, (1, 3, 9)), _ct()
    msg = "resstack_x3: unaligned rows, more than 64 utterances or an utterance shorter than the reflection pad"
    _raises(msg, 3, 48, _xrows(96, (8,)), blocks=blocks, ct=ct, mul=2)
    _raises("resstack_x3: fused ConvTranspose arguments", 3, 48, _xrows(96, (20,)), blocks=blocks, ct=ct, mul=1)
    _raises("resstack_x3: fused ConvTranspose only at C = 48", 3, 96, _xrows(192, (20,)), blocks=_blocks(96, (1, 3, 9)),
            ct=_ct(96), mul=2)


# =====================================================================================================
# Output kernels: kind 4 (output conv + PQMF synthesis) and kind 5 (full-band output conv)
# =====================================================================================================
EPS1 = 2.0 ** -23  # one float32 spacing at the output scale: tanh and the synthesis of it lie in [-1, 1]


@pytest.mark.parametrize("C", [32, 48])
def test_out_pqmf_band_lengths(C):
    """L = 4 (the shortest ReflectionPad1d(3) takes), 7, 8, 9 (the synthesis halo), TB - 1, TB, TB + 1, 2 TB + 1;
    then B = 3 ragged with maxL two whole tiles past the shortest row: exact zeros from 4 L to 4 maxL."""
    tb = _tq(4, C)
    assert tb == TQ_PQMF, f"out_pqmf_kernel<{C}> reports tq {tb}"
    wo, bo = _outw(C, 4)
    G = _G()
    assert G.shape == (4, 63)
    lens = (4, 7, 8, 9, tb - 1, tb, tb + 1, 2 * tb + 1)
    rows = _xrows(C, lens)
    ref, e32, _ = _oracle(("pq", C, lens), lambda dt: V.out_pqmf(rows, wo, bo, G, dt))
    for b, r in enumerate(rows):
        o, tq, flag = run(4, C, [r], out=(wo, bo), G=G)
        assert tq == tb and flag == 0
        within(f"pqmf C {C}", 4, o, [ref[b]], [e32[b]], floor=EPS1)
    lens3 = (tb + 5, 7, 2 * tb + 1)
    rows3 = _xrows(C, lens3, seed=1)
    ref3, e3, _ = _oracle(("pq", C, lens3), lambda dt: V.out_pqmf(rows3, wo, bo, G, dt))
    maxL = 2 * tb + 9
    o, tq, flag = run(4, C, rows3, out=(wo, bo), G=G, max_q=maxL)
    assert tq == tb and flag == 0 and all(r.shape == (1, 4 * maxL) for r in o)
    within(f"pqmf ragged C {C}", 4, [r[:, :4 * n] for r, n in zip(o, lens3)], ref3, e3, floor=EPS1)
    for r, n in zip(o, lens3):
        assert not r[:, 4 * n:].any() and not np.signbit(r[:, 4 * n:]).any(), "zeros from 4 L to 4 maxL"
    _raises("fused output/PQMF shape not covered", 4, C, rows3, out=(wo, bo), G=G, max_q=maxL, yb_extra=1)
    _raises("fused output/PQMF shape not covered", 4, 64, _xrows(64, (8,)), out=_outw(64, 4), G=G)


@pytest.mark.parametrize("C", [32, 64])
def test_out_conv1_lengths_and_store_forms(C):
    """L = 4, 15, 16, 17, 19, 20, 21, 36 (a thread's 16 positions and the 16-byte loads' 4 + 16 + 4 window),
    4095, 4096, 4097 (a workgroup's 4096); aligned (16-byte loads and stores away from the row ends) and with
    an odd channel stride (per-element form), bit-identical; then B = 3 ragged."""
    per = _tq(5, C)
    assert per == TQ_OUT1, f"out_conv1_kernel reports {per} positions per workgroup"
    wo, bo = _outw(C, 1)
    lens = (4, 15, 16, 17, 19, 20, 21, 36, per - 1, per, per + 1)
    rows = _xrows(C, lens)
    ref, e32, _ = _oracle(("o1", C, lens), lambda dt: V.out_bands(rows, wo, bo, dt))
    for b, r in enumerate(rows):
        o, tq, flag = run(5, C, [r], out=(wo, bo))
        assert tq == per and flag == 0
        within(f"out_conv1 C {C}", 5, o, [ref[b]], [e32[b]], floor=EPS1)
        alt = run(5, C, [r], out=(wo, bo), x_extra=1)[0]
        _same(f"out_conv1 C {C} L {lens[b]}: odd channel stride vs aligned", alt, o)
    lens3 = (per + 21, 4, 36)
    rows3 = _xrows(C, lens3, seed=1)
    ref3, e3, _ = _oracle(("o1", C, lens3), lambda dt: V.out_bands(rows3, wo, bo, dt))
    o = run(5, C, rows3, out=(wo, bo))[0]
    within(f"out_conv1 ragged C {C}", 5, o, ref3, e3, floor=EPS1)
    _same(f"out_conv1 ragged C {C}: odd channel stride vs aligned", run(5, C, rows3, out=(wo, bo), x_extra=1)[0], o)


# =====================================================================================================
# Range flag, kinds 1-3: NaN or out-of-range operand -> flag
# =====================================================================================================
# The float64 oracle alone decides the expectation: its largest operand is below 65504 / 4 in every flag-0 case
# (asserted in block_case / stack_case / ct_case above, whose sources are NaN everywhere outside the rows) and
# above 2 x 65504 in every flag-1 case where the operand is computed (h, x_1 .. x_2, the ConvTranspose's
# output). Where the operand is the input itself (the 1e5 spike) nothing is rounded on the way to the check,
# so the oracle's maximum only has to be that value, above 65504.
def _spiked(rows, b, pos, value):
    rows = [r.copy() for r in rows]
    rows[b][3, pos] = value
    return rows


def _flag1(what, kind, C, rows, fn, need, **kw):
    with np.errstate(invalid="ignore", over="ignore"):
        _, mx = fn(np.float64)
    if need == "nan":
        assert np.isnan(mx), f"{what}: oracle's largest operand {mx}"
    else:  # an inf met twice with opposite signs is a NaN: as far outside as it gets
        assert np.isnan(mx) or mx > need, f"{what}: the oracle's largest operand {mx} is not clearly outside the f16 range"
    _, tq, flag = run(kind, C, rows, **kw)
    print(f"{what}: kind {kind} oracle's largest operand {mx:.4g} flag {flag}")
    assert flag == 1, f"{what}: kind {kind} range flag {flag}"


X_VALUES = [("1e5", 1e5, 1e5 - 1), ("inf", np.inf, 2 * F16_MAX), ("nan", np.nan, "nan")]


@pytest.mark.parametrize("C", [32, 48, 96, 256])
@pytest.mark.parametrize("name, value, need", X_VALUES)
def test_range_flag_block_input(C, name, value, need):
    """In x inside a tile; and at position TQ of a row of TQ + 1, which tile 0 stages only as its halo (and the
    one-position tile 1 as its centre)."""
    tq = _tq(1, C)
    d = 3
    blk = _blocks(C, (d,))
    for what, lens, b, pos in (("inside a tile", (tq + 9,), 0, 5), ("second row, halo of tile 0", (20, tq + 1), 1, tq)):
        rows = _spiked(_xrows(C, lens), b, pos, np.float32(value))
        _flag1(f"block C {C} x = {name} {what}", 1, C, rows, lambda dt: V.resblock(rows, *blk[0], dt), need, blocks=blk)
    assert run(0, C, rows, blocks=blk)[2] == 0  # the fp32 kernel has no flag


@pytest.mark.parametrize("C", [32, 48, 96, 256])
def test_range_flag_block_hidden_activation(C):
    """wd scaled by 1e5 (every weight still inside the f16 range): x stays small, only h leaves the range."""
    tq = _tq(1, C)
    blk = _blocks(C, (1,))
    big = [(blk[0][0] * np.float32(1e5),) + blk[0][1:]]
    assert np.abs(big[0][0]).max() < F16_MAX
    rows = _xrows(C, (2 * tq + 1,))
    assert max(np.abs(r).max() for r in rows) < F16_MAX / 4
    _flag1(f"block C {C} h", 1, C, rows, lambda dt: V.resblock(rows, *big[0], dt), 2 * F16_MAX, blocks=big)


@pytest.mark.parametrize("C", [48, 96])
def test_range_flag_stack(C):
    tq = _tq(2, C)
    blocks = _blocks(C, (1, 3, 9))
    base = _xrows(C, (tq + 30, 40))
    for name, value, need in X_VALUES:
        for what, b, pos in (("inside a tile", 0, 5), ("halo of tile 0", 0, tq + 3)):
            rows = _spiked(base, b, pos, np.float32(value))
            _flag1(f"stack C {C} x = {name} {what}", 2, C, rows, lambda dt: V.resstack(rows, blocks, dt), need, blocks=blocks)
    big = [(blocks[0][0] * np.float32(1e5),) + blocks[0][1:]] + blocks[1:]
    _flag1(f"stack C {C} h of block 0", 2, C, base, lambda dt: V.resstack(base, big, dt), 2 * F16_MAX, blocks=big)
    # block 1's output: W_1x1 and W_sc of block 1 scaled, everything before it inside the range
    b1 = blocks[1]
    big = [blocks[0], (b1[0], b1[1], b1[2] * np.float32(5e4), b1[3], b1[4] * np.float32(5e4), b1[5], b1[6]), blocks[2]]
    assert max(np.abs(big[1][2]).max(), np.abs(big[1][4]).max()) < F16_MAX
    h1_in = V.resstack(base, [blocks[0]])[0]
    assert V.resblock(h1_in, *blocks[1])[1] < F16_MAX / 4  # x_0, h_0, x_1 and h_1 stay small
    _flag1(f"stack C {C} output of block 1", 2, C, base, lambda dt: V.resstack(base, big, dt), 2 * F16_MAX, blocks=big)


def test_range_flag_fused_conv_transpose():
    blocks, ct = _blocks(48, (1, 3, 9)), _ct()
    base = _xrows(96, (130, 20))
    for name, value, need in X_VALUES:
        for what, pos in (("inside a tile", 5), ("halo of tile 0", 106)):
            rows = _spiked(base, 0, pos, np.float32(value))
            _flag1(f"ct x = {name} {what}", 3, 48, rows, lambda dt: V.ct_resstack(rows, ct[0], ct[1], blocks, dt), need,
                   blocks=blocks, ct=ct, mul=2)
    bigct = (ct[0] * np.float32(1e5), ct[1])
    assert np.abs(bigct[0]).max() < F16_MAX and max(np.abs(r).max() for r in base) < F16_MAX / 4
    _flag1("ct output of the ConvTranspose", 3, 48, base, lambda dt: V.ct_resstack(base, bigct[0], bigct[1], blocks, dt),
           2 * F16_MAX, blocks=blocks, ct=bigct, mul=2)


def test_zz_largest_ratios():
    """The largest error / e32 per kind over this run (the figures of DESIGN.md 4.4); no new assertion."""
    for kind in sorted(ratios):
        print(f"largest ratio kind {kind}: {ratios[kind]:.2f}")
    assert all(r <= 8 for r in ratios.values())
