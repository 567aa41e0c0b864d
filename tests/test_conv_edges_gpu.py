"""The generic conv kernels (conv.hip fp32 MFMA, conv_x3.hip split-f16 MFMA) on their own, through
tts_test_conv (pack_conv / pack_convT / run_conv as shipped), against oracle/conv_np.py in float64
(pinned to torch by tests/test_conv_oracle.py): tile classes and taps, the chunk pipeline, dilation,
tile and deal edges, padding, layouts, epilogues, the phase-merged ConvTranspose and the range flag.

Every case runs in "f32" and "x3" GEMM mode and asserts the kernel the library reports. Every call's
source is NaN past each row's length (and in the channel padding of a time-major source), and every
output buffer carries a sentinel in each element the call must not write (past a row's positions,
between rows, in a margin on both sides); both are checked on every call.

Tolerance: e32 = max |oracle(float32) - oracle(float64)| of the case, the oracle's
float32 form being a plain term-by-term float32 sum; every output element of either kernel is within
8 x e32 of the float64 oracle. e32 is taken per case, not per output channel: rows here have 1 to a few
hundred positions, so a channel's own maximum is a sample of a handful of values (one value at length
1, where it can be exactly 0) and varies several-fold between channels of equal statistics. The
split-f16 error is also at most 2 x the fp32 kernel's on the same case plus 2e-6 x max(1, max |ref|)
(the relation and absolute term of test_mbmelgan_split_f16_equals_fp32_path_and_oracle, whose outputs
lie in [-1, 1], scaled to the case's outputs). Each comparison prints error, e32 and ratio first.
Weights are N(0, 1) / sqrt(Cin K), inputs N(0, 1) unless a case says otherwise."""
import numpy as np
import pytest
import torch

from oracle import conv_np as O

pytestmark = pytest.mark.gpu

SENT = np.float32(-12345.678)
MARGIN = 64  # sentinel elements on both sides of the output (a multiple of 4: keeps the alignment)
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


def _engine(mode):
    from tts_amd._lib import get_engine
    eng = get_engine(_dev())
    eng.set_gemm_mode(mode)
    return eng


@pytest.fixture(autouse=True)
def _default_mode_after():
    yield
    _engine("x3")


def case(**kw):
    c = dict(Cin=32, Cout=64, K=3, dil=1, lens=(33,), pad_left=None, pad_mode=0, rep_pad=0, len_add=0, act=0, epi=0,
             nphase=1, resid=None, resid_rows=0, aux=False, src="bct", out="bct", split=0, src_cpad=0, out_tpad=3,
             out_off=0, gap=5, seed=0, u=0, merged=False, xform=None, wform=None, mul=1)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    c["lens"] = tuple(int(n) for n in c["lens"])
    if c["pad_left"] is None:
        c["pad_left"] = ((c["K"] - 1) * c["dil"] // 2,) * c["nphase"]
    c["pad_left"] = tuple(c["pad_left"])
    return c


def _out_rows(c):
    return c["Cout"] // 2 if c["epi"] in (3, 4, 6) else c["Cout"]


def _prepare(c):
    """Inputs and both oracle runs of a case, computed once."""
    key = tuple(sorted((k, v) for k, v in c.items() if k not in ("src", "out", "src_cpad", "out_tpad", "out_off", "gap",
                                                                  "merged", "split")))
    if key in _cache:
        return _cache[key]
    rs = np.random.RandomState(c["seed"] + 7 * c["Cin"] + 13 * c["Cout"] + c["K"])
    Cin, Cout, K, u = c["Cin"], c["Cout"], c["K"], c["u"]
    if u:
        w = rs.normal(0, 1 / np.sqrt(2 * Cin), (Cin, Cout, 2 * u)).astype(np.float32)
    else:
        shape = (Cout, Cin, K) if c["nphase"] == 1 else (c["nphase"], Cout, Cin, K)
        w = rs.normal(0, 1 / np.sqrt(Cin * K), shape).astype(np.float32)
    bias = rs.normal(0, 0.5, Cout).astype(np.float32)
    src_len = [n if c["rep_pad"] else (n + c["len_add"]) * c["mul"] for n in c["lens"]]
    xs = [rs.normal(0, 1, (Cin, n)).astype(np.float32) for n in src_len]
    if c["xform"]:
        xs = [c["xform"](x, rs) for x in xs]
    if c["wform"]:
        w = c["wform"](w)
    Tout = [(n + c["len_add"]) * c["mul"] * (u if u else c["nphase"]) for n in c["lens"]]
    rrows = {4: Cout // 2, 5: Cout}.get(c["epi"], Cout)
    resid = [rs.normal(0, 1, (rrows, t)).astype(np.float32) for t in Tout] if (c["resid"] or c["epi"] in (4, 5)) else None
    aux = None
    if c["epi"] == 5:
        aux = rs.normal(0, 0.5, (Cout, 6)).astype(np.float32)
    elif c["aux"]:
        aux = rs.normal(0, 0.5, (len(xs), Cout)).astype(np.float32)
    refs = []
    for dt in (np.float64, np.float32):
        if u:
            refs.append([O.conv_transpose1d(x, w, bias, u, dt, act=c["act"]) for x in xs])
        else:
            refs.append(O.conv_rows(xs, w, bias, c["lens"], dt, dil=c["dil"], pad_left=c["pad_left"], pad_mode=c["pad_mode"],
                                    rep_pad=c["rep_pad"], len_add=c["len_add"], in_mul=c["mul"], q_mul=c["mul"],
                                    out_mul=c["nphase"], act=c["act"],
                                    epi=c["epi"], resid=resid, resid_rows=c["resid_rows"], aux=aux))
    with np.errstate(invalid="ignore"):  # the range flag cases put inf / NaN in
        e32 = max([float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(refs[1], refs[0]) if b.size] + [0.0])
    p = dict(w=w, bias=bias, xs=xs, resid=resid, aux=aux, ref=refs[0], e32=e32, Tout=Tout)
    _cache[key] = p
    return p


def _rows_to_device(rows, layout, cpad, fill=np.nan):
    """rows[b] (C, T_b) -> (tensor, (address, strides)) in (B, C, T) or (B, T, C + cpad), 3 spare
    positions per row; everything that is not a row's data is `fill`."""
    B, C, Tn = len(rows), rows[0].shape[0], max(r.shape[1] for r in rows) + 3
    if layout == "bct":
        a = np.full((B, C, Tn), fill, np.float32)
        for b, r in enumerate(rows):
            a[b, :, :r.shape[1]] = r
        st = (C * Tn, Tn, 1)
    else:
        Cs = C + cpad
        a = np.full((B, Tn, Cs), fill, np.float32)
        for b, r in enumerate(rows):
            a[b, :r.shape[1], :C] = r.T
        st = (Tn * Cs, 1, Cs)
    t = torch.from_numpy(a).to(_dev())
    return t, (t.data_ptr(), st)


def run(c, mode, p=None):
    """One call -> (rows of the output as numpy (rows, Tout_b), (ran_x3, tq, flag)); checks the sentinels.
    p: the prepared inputs, when they are not the case's own (one row of a batch's)."""
    p = p or _prepare(c)
    eng = _engine(mode)
    keep = []
    C0 = c["split"]
    if C0:
        t0, s0 = _rows_to_device([x[:C0] for x in p["xs"]], c["src"], c["src_cpad"])
        t1, s1 = _rows_to_device([x[C0:] for x in p["xs"]], "btc" if c["src"] == "bct" else "bct", 0)
        keep += [t0, t1]
        src, src2 = s0 + (C0, c["act"]), s1 + (c["Cin"] - C0, c["act"])
    else:
        t0, s0 = _rows_to_device(p["xs"], c["src"], c["src_cpad"])
        keep.append(t0)
        src, src2 = s0 + (c["Cin"], c["act"]), None
    rows, Tout, B = _out_rows(c), p["Tout"], len(c["lens"])
    Tn = max(Tout) + c["out_tpad"]
    if c["out"] == "bct":
        oc, ot, ob = Tn, 1, rows * Tn + c["gap"]
    else:
        Cs = rows + 3
        oc, ot, ob = 1, Cs, Tn * Cs + c["gap"]
    base = MARGIN + c["out_off"]
    flat = torch.full((base + B * ob + MARGIN,), float(SENT), dtype=torch.float32, device=_dev())
    out = (flat.data_ptr() + 4 * base, (ob, oc, ot))
    resid = None
    if p["resid"] is not None:
        lay = c["resid"] or c["out"]
        tr, resid = _rows_to_device(p["resid"], lay, 1)
        keep.append(tr)
    aux, auxb = None, 0
    if p["aux"] is not None:
        ta = torch.from_numpy(p["aux"]).to(_dev())
        keep.append(ta)
        aux, auxb = ta.data_ptr(), (c["Cout"] if c["epi"] == 3 else 0)
    u = c["u"]
    kw = dict(K=c["K"], dil=c["dil"], nphase=c["nphase"], pad_left=c["pad_left"], src2=src2, resid=resid,
              resid_rows=c["resid_rows"], aux=aux, auxb=auxb, len_add=c["len_add"], rep_pad=c["rep_pad"],
              pad_mode=c["pad_mode"], epi=c["epi"], out_mul=c["nphase"])
    kw.update(in_mul=c["mul"], q_mul=c["mul"])
    max_q = max(n + c["len_add"] for n in c["lens"]) * c["mul"]
    if u:
        kw.update(transposed=True, nphase=u, out_mul=1 if c["merged"] else u, merged_u=u if c["merged"] else 0)
        max_q += 1 if c["merged"] else 0
    info = eng.conv_test(p["w"], p["bias"], c["lens"], src, out, max_q, _dev(), **kw)
    h = flat.cpu().numpy()
    written = np.zeros(h.shape, bool)
    outs = []
    for b in range(B):
        idx = base + b * ob + np.arange(rows)[:, None] * oc + np.arange(Tout[b])[None, :] * ot
        outs.append(h[idx])
        written[idx] = True
    assert (h[~written].view(np.uint32) == SENT.view(np.uint32)).all(), "the call wrote outside its result"
    return outs, info


def _err(outs, ref):
    return max([float(np.abs(o.astype(np.float64) - r).max()) for o, r in zip(outs, ref) if r.size] + [0.0])


def check(what, c, x3=True):
    """Both modes against the float64 oracle; returns the split-f16 mode's output rows and tile width."""
    p = _prepare(c)
    o32, (r32, tq32, f32) = run(c, "f32")
    o16, (r16, tq16, f16) = run(c, "x3")
    e32, scale = p["e32"], max([1.0] + [float(np.abs(r).max()) for r in p["ref"] if r.size])
    k32, k16 = _err(o32, p["ref"]), _err(o16, p["ref"])
    print(f"{what}: f32 kernel tq {tq32} err {k32:.3e} ratio {k32 / max(e32, 1e-30):.2f} | x3 mode "
          f"{'split-f16' if r16 else 'fp32'} tq {tq16} err {k16:.3e} ratio {k16 / max(e32, 1e-30):.2f} | e32 {e32:.3e}")
    assert not r32 and f32 == 0, f"{what}: f32 mode ran {'split-f16' if r32 else 'fp32'}, flag {f32}"
    assert r16 == x3, f"{what}: x3 mode ran {'split-f16' if r16 else 'fp32'}"
    assert f16 == 0, f"{what}: range flag {f16}"
    for o in o32 + o16:
        assert np.isfinite(o).all(), f"{what}: non-finite output"
    assert k32 <= 8 * e32, f"{what}: fp32 kernel {k32:.3e} > 8 x {e32:.3e}"
    assert k16 <= 8 * e32, f"{what}: x3 mode {k16:.3e} > 8 x {e32:.3e}"
    assert k16 <= 2 * k32 + 2e-6 * scale, f"{what}: split-f16 {k16:.3e} vs fp32 kernel {k32:.3e}"
    return o16, tq16


def _raises(c, mode, text):
    with pytest.raises(RuntimeError) as ei:
        run(c, mode)
    assert text in str(ei.value), str(ei.value)


# ---- tile classes x taps ----
X3_CLASSES = [128, 256, 192, 96, 64, 320, 80, 160, 48]


@pytest.mark.parametrize("Cout", X3_CLASSES + [16, 4, 1])
def test_tile_classes_and_taps(Cout):
    """Cin = 96 (three 32-channel chunks); rows straddle the class's tile widths (48 / 64 / 128 / 256)."""
    x3 = Cout in X3_CLASSES
    lens = ((63, 65, 49) if Cout in (128, 256, 192) else (127, 129, 65)) if x3 else (255, 257, 3)
    for K in (1, 2, 3, 5, 7):
        check(f"Cout {Cout} K {K}", case(Cin=96, Cout=Cout, K=K, lens=lens), x3=x3)


# ---- chunk pipeline ----
@pytest.mark.parametrize("Cout", [128, 80])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_chunk_pipeline(Cout, K):
    """NCH = ceil(Cin / 32) = 1 .. 5 and partial last chunks (Cin = 16, 48, 80)."""
    for Cin in (16, 32, 48, 64, 80, 96, 128, 160):
        check(f"Cout {Cout} K {K} Cin {Cin}", case(Cin=Cin, Cout=Cout, K=K, lens=(70, 33)))


# ---- dilation ----
@pytest.mark.parametrize("K, dil", [(2, 1), (2, 7), (3, 1), (3, 3)])
def test_dilation(K, dil):
    for Cout in (128, 64):
        for mode in (0, 1):
            check(f"K {K} dil {dil} Cout {Cout} pad mode {mode}",
                  case(Cin=64, Cout=Cout, K=K, dil=dil, lens=(140, 20), pad_mode=mode))


@pytest.mark.parametrize("K, dil", [(3, 4), (2, 8), (5, 2)])
def test_span_of_eight_raises(K, dil):
    for mode in ("f32", "x3"):
        _raises(case(Cin=32, Cout=64, K=K, dil=dil, lens=(40,)), mode, "receptive span too large")


# ---- tile and deal edges ----
EDGE_LENS = [1, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257]


@pytest.mark.parametrize("Cout", [128, 64, 48, 16])
def test_single_rows_at_every_tile_width(Cout):
    """Boundaries of TQ = 48 / 64 (Cout 128, either width the cost model picks), 128 (64, 48) and of
    the fp32 kernel's 64 / 128 (48) / 256 (16)."""
    for L in EDGE_LENS:
        check(f"Cout {Cout} L {L}", case(Cin=32, Cout=Cout, K=3, lens=(L,), pad_mode=2), x3=Cout != 16)


def _batch_rows_equal_single_rows(what, c):
    """check(), then per mode: the same call twice and every row's own B = 1 call are bit-identical."""
    o16, tq = check(what, c)
    p = _prepare(c)
    for mode in ("f32", "x3"):
        outs, info = run(c, mode)
        again, info2 = run(c, mode)
        assert info == info2
        for b, n in enumerate(c["lens"]):
            assert np.array_equal(outs[b], again[b]), f"{what} {mode}: row {b} differs between two equal calls"
            one = dict(p, xs=[p["xs"][b]], ref=[p["ref"][b]], Tout=[p["Tout"][b]],
                       resid=None if p["resid"] is None else [p["resid"][b]])
            single, _ = run(dict(c, lens=(n,)), mode, one)
            assert np.array_equal(single[0], outs[b]), f"{what} {mode}: row {b} differs from its B = 1 call"
    return tq


@pytest.mark.parametrize("tiles", [1, 7, 8, 9, 17])
def test_ragged_batches_by_tile_count(tiles):
    """nq nco B tiles in the split-f16 kernel's deal (8 XCDs): Cout 64 (one 64-row tile, TQ 128) and
    Cout 192 (one 192-row tile, TQ 64). The first and the last tile of each list hold positions (the
    last row's last tile), so a deal that drops or doubles an end of the list shows."""
    for Cout, TQ in ((64, 128), (192, 64)):
        lens = {1: (TQ - 7,), 7: (TQ, 1, TQ - 1, 5, 17, 2, TQ // 2), 8: (3, TQ, 1, TQ - 1, 5, 17, 2, TQ // 2),
                9: (TQ + 2, 1, 2 * TQ + 9), 17: tuple([TQ, 1, 9, TQ - 1] * 4 + [33])}[tiles]
        nq = -(-max(lens) // TQ)
        assert nq * len(lens) == tiles
        tq = _batch_rows_equal_single_rows(f"tiles {tiles} Cout {Cout}", case(Cin=64, Cout=Cout, K=3, lens=lens, seed=tiles))
        assert tq == TQ


@pytest.mark.parametrize("Cout", [128, 64, 160])
def test_three_tile_row_beside_one_position_rows(Cout):
    """The q0 >= Lq return: tiles 1 and 2 of the short rows are dealt and leave at once."""
    _batch_rows_equal_single_rows(f"Cout {Cout}", case(Cin=48, Cout=Cout, K=5, lens=(1, 3 * 128 - 5, 1, 1), pad_mode=2))


# ---- padding ----
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_padding_modes_and_asymmetric_pad_left(K, mode):
    span = K - 1
    for pad in (0, span // 2, span):
        check(f"K {K} mode {mode} pad_left {pad}", case(Cin=32, Cout=64, K=K, lens=(140, 9), pad_left=(pad,), pad_mode=mode))


@pytest.mark.parametrize("K", [3, 5, 7])
def test_rows_shorter_than_the_span(K):
    for mode in (0, 2):
        for Cout in (64, 128):
            check(f"K {K} mode {mode} Cout {Cout} L 1, 2", case(Cin=32, Cout=Cout, K=K, lens=(1, 2), pad_mode=mode))


@pytest.mark.parametrize("K, pad", [(7, 3), (5, 2), (3, 2), (7, 6)])
def test_reflect_at_length_pad_plus_one(K, pad):
    check(f"K {K} pad {pad}", case(Cin=32, Cout=64, K=K, lens=(pad + 1, pad + 2), pad_left=(pad,), pad_mode=1))


@pytest.mark.parametrize("src", ["bct", "btc"])
def test_vocoder_first_conv_rep_pad(src):
    """80 -> 384, k7, ReflectionPad1d(3) over the mel replicate-padded by 2 on each side."""
    check(f"rep_pad src {src}", case(Cin=80, Cout=384, K=7, lens=(12, 1, 50), pad_left=(3,), pad_mode=1, rep_pad=2,
                                     len_add=4, src=src))


@pytest.mark.parametrize("Cout, L", [(192, 200), (64, 400), (128, 200)])
def test_interior_tile_between_edge_tiles(Cout, L):
    for mode in (0, 1):
        check(f"Cout {Cout} L {L} mode {mode}", case(Cin=64, Cout=Cout, K=5, lens=(L,), pad_mode=mode))


# ---- layouts ----
@pytest.mark.parametrize("src", ["bct", "btc"])
@pytest.mark.parametrize("out", ["bct", "btc"])
def test_source_and_output_layouts(src, out):
    for Cin in (64, 48):  # 48: the time-major loads of the last chunk reach past Cin
        for act in (0, 1):
            check(f"src {src} out {out} Cin {Cin} act {act}",
                  case(Cin=Cin, Cout=128, K=3, lens=(70, 9), src=src, out=out, act=act))


def test_time_major_source_with_odd_stride_runs_fp32():
    """A (B, T, C) view whose time stride is no multiple of 4: no 16-byte loads, so run_conv takes the
    fp32 kernel in x3 mode."""
    check("btc stride Cin + 1", case(Cin=32, Cout=64, K=3, lens=(70, 9), src="btc", src_cpad=1), x3=False)
    check("btc stride Cin + 4", case(Cin=32, Cout=64, K=3, lens=(70, 9), src="btc", src_cpad=4), x3=True)


@pytest.mark.parametrize("src", ["bct", "btc"])
def test_two_sources_run_fp32(src):
    check(f"two sources, first {src}", case(Cin=64, Cout=64, K=3, lens=(70, 9), split=16, src=src, act=1), x3=False)
    check(f"two sources 32 + 32, first {src}", case(Cin=64, Cout=128, K=5, lens=(70, 9), split=32, src=src), x3=False)


@pytest.mark.parametrize("u", [2, 4, 8])
def test_polyphase_conv_transpose(u):
    """pack_convT's u polyphase 2-tap convs (out_mul = u) against conv_transpose1d."""
    for Cout in (64, 24):
        check(f"u {u} Cout {Cout}", case(Cin=64, Cout=Cout, u=u, lens=(37, 1, 130), act=1), x3=Cout == 64)


def test_length_multipliers():
    """in_mul = q_mul = 8 over base lengths, as the vocoder's later stages run: Lin = Lq = 8 (lens + len_add)."""
    check("mul 8", case(Cin=64, Cout=64, K=3, lens=(17, 2, 9), mul=8, pad_mode=1, act=1))
    check("mul 8 len_add 2", case(Cin=32, Cout=128, K=7, lens=(5, 1), mul=8, len_add=2, pad_mode=1))
    check("mul 4 polyphase u 2", case(Cin=64, Cout=64, u=2, lens=(17, 2, 33), mul=4, act=1))
    c = case(Cin=64, Cout=64, u=2, lens=(17, 2, 33), mul=4, act=1, merged=True, out_tpad=4, gap=8)
    outs, info = run(c, "x3")
    p = _prepare(c)
    k = _err(outs, p["ref"])
    print(f"mul 4 merged u 2: tq {info[1]} err {k:.3e} e32 {p['e32']:.3e} ratio {k / p['e32']:.2f}")
    assert info[0] and info[2] == 0 and k <= 8 * p["e32"]


def test_generic_phases_with_three_taps():
    check("nphase 2 K 3", case(Cin=32, Cout=64, K=3, nphase=2, pad_left=(1, 2), lens=(70, 9)))


@pytest.mark.parametrize("out, resid", [("bct", "btc"), ("btc", "bct"), ("bct", "bct")])
def test_residual_layouts_and_resid_rows(out, resid):
    for Cout in (128, 80):
        for rows in (0, Cout - 5, 16):
            check(f"out {out} resid {resid} Cout {Cout} resid_rows {rows}",
                  case(Cin=64, Cout=Cout, K=3, lens=(70, 9), out=out, resid=resid, resid_rows=rows, epi=1))


# ---- epilogues ----
@pytest.mark.parametrize("epi, aux", [(1, False), (2, False), (3, False), (3, True), (4, False), (5, False), (6, False)])
def test_epilogue_forms(epi, aux):
    for Cout in (128, 160):
        check(f"epi {epi} aux {aux} Cout {Cout}", case(Cin=64, Cout=Cout, K=3, lens=(70, 9), epi=epi, aux=aux))
    if epi >= 3:  # the 16-row tile, half empty: pairs and mixing groups end at Cout
        check(f"epi {epi} aux {aux} Cout 8", case(Cin=64, Cout=8, K=3, lens=(70, 9), epi=epi, aux=aux), x3=False)


# ---- phase-merged ConvTranspose ----
MERGED = [(2, 64), (2, 24), (4, 48), (4, 20), (8, 16), (8, 12)]
MERGED_LENS = [(1,), (47,), (48,), (49,), (63,), (64,), (65,), (127,), (128,), (129,), (50, 1, 129, 64)]


@pytest.mark.parametrize("u, Cout", MERGED)
def test_merged_conv_transpose(u, Cout):
    """One GEMM of u Cout rows over inputs 0 .. L (Lq = L + 1): L = 1, TQ - 1, TQ, TQ + 1 for each width
    the merged row count may launch (48 / 64 / 128), and a ragged batch; vector stores, then the scalar
    form (odd row stride; output 4 bytes off 16-byte alignment), bit-identical. Split-f16 only: f32
    mode refuses it."""
    for lens in MERGED_LENS:
        c = case(Cin=64, Cout=Cout, u=u, lens=lens, act=1, merged=True, out_tpad=4 - (max(lens) * u) % 4, gap=8)
        p = _prepare(c)
        _raises(c, "f32", "phase-merged ConvTranspose runs on split-f16 weights only")
        outs, (x3, tq, flag) = run(c, "x3")
        k = _err(outs, p["ref"])
        print(f"merged u {u} Cout {Cout} L {lens}: tq {tq} err {k:.3e} e32 {p['e32']:.3e} ratio {k / max(p['e32'], 1e-30):.2f}")
        assert x3 and flag == 0 and k <= 8 * p["e32"]
        # the polyphase form of the same layer in fp32: the relation between the two kernels
        o32, (r32, _, _) = run(dict(c, merged=False), "f32")
        assert not r32 and k <= 2 * _err(o32, p["ref"]) + 2e-6 * max(1.0, max(float(np.abs(r).max()) for r in p["ref"]))
        for what, alt in (("odd row stride", dict(c, out_tpad=c["out_tpad"] + 1)), ("offset pointer", dict(c, out_off=1))):
            scalar, info = run(alt, "x3")
            assert info == (True, tq, 0)
            for a, b in zip(scalar, outs):
                assert np.array_equal(a, b), f"merged u {u} Cout {Cout} L {lens}: {what} differs from the vector form"


# ---- strided outputs ----
@pytest.mark.parametrize("out", ["bct", "btc"])
def test_strided_output_rows_keep_their_gaps(out):
    check(f"out {out} gap 37", case(Cin=32, Cout=96, K=3, lens=(130, 7, 64), out=out, gap=37, out_tpad=9))


# ---- range flag ----
BELOW = np.nextafter(np.float32(65504), np.float32(0))


def _spike(value, pos=(3, 5)):
    def f(x, rs):
        x = x.copy()
        x[pos] = value
        return x
    return f


def _flag_case(value):
    return case(Cin=32, Cout=64, K=3, lens=(40,), xform=_spike(value))


@pytest.mark.parametrize("value, flag", [(65504.0, 1), (-65504.0, 1), (float(BELOW), 0), (float("nan"), 1), (float("inf"), 1)])
def test_range_flag(value, flag):
    c = _flag_case(np.float32(value))
    if flag == 0:
        check(f"activation {value!r}", c)
        return
    outs, (x3, tq, got) = run(c, "x3")
    print(f"activation {value!r}: split-f16 {x3} flag {got}")
    assert x3 and got == 1
    assert run(c, "f32")[1] == (False, 64, 0)


def test_masked_values_do_not_set_the_flag():
    """Zero padding, channels past Cin and data past a row's length are NaN in every call of this file;
    here also 65504 right past each row's end and in the channel padding."""
    for src in ("bct", "btc"):
        c = case(Cin=48, Cout=64, K=5, lens=(40, 7), src=src, src_cpad=4)
        p = _prepare(c)
        eng = _engine("x3")
        t0, s0 = _rows_to_device(p["xs"], src, 4, fill=65504.0)
        flat = torch.full((2 * 64 * 50,), float(SENT), dtype=torch.float32, device=_dev())
        info = eng.conv_test(p["w"], p["bias"], c["lens"], s0 + (48, 0), (flat.data_ptr(), (64 * 50, 50, 1)), 40, _dev(),
                             K=5, pad_left=(2,))
        assert info[0] and info[2] == 0
        h = flat.cpu().numpy().reshape(2, 64, 50)
        assert max(np.abs(h[b, :, :n] - p["ref"][b]).max() for b, n in enumerate(c["lens"])) <= 8 * p["e32"]


def test_weight_at_f16_max_leaves_no_split_weights():
    def big(w):
        w = w.copy()
        w[1, 2, 0] = 65504.0
        return w
    check("weight 65504", case(Cin=32, Cout=64, K=3, lens=(40,), wform=big), x3=False)


def test_log_uniform_magnitudes():
    """|x| log-uniform over 2^-20 .. 2^15: the lo half of a split value is an f16 subnormal below ~6e-5."""
    def logu(x, rs):
        return (np.sign(x) * np.exp2(rs.uniform(-20, 15, x.shape))).astype(np.float32)
    for Cout, Cin, K in ((128, 96, 5), (80, 48, 1), (64, 160, 7)):
        check(f"log-uniform Cout {Cout} Cin {Cin} K {K}", case(Cin=Cin, Cout=Cout, K=K, lens=(70, 33), xform=logu))
