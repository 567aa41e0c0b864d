"""GPU parity of ``GlowTts.forward`` (eval) against the reference's own ``forward`` (fixtures:
tests/golden/make_glow_forward_golden.py; every row there is the reference's B = 1 call).

The alignment is exact: the fixture rows meet ``margin >= 10 x qdrift`` (asserted by the generator
and by test_glow_forward_host.py). ``z``, ``logp`` and ``logdet`` are scored against the reference's
fp64 run; the bound is 8 x the reference's own fp32-vs-fp64 error for that quantity and row (the
factor of DESIGN.md 4.7 / 4.8), for ``z`` never tighter than the 1e-4 of the other Glow tests.
Measured figures are printed before each assertion and recorded in DESIGN.md 4.9."""
import numpy as np
import pytest
import torch

from helpers import load_fixture
from tts_amd.spec import GlowConfig, glow_spec
from tts_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4
FACTOR = 8.0
ROWS = ((1, 2), (5, 11), (8, 8), (70, 150))
PAD = 50.0  # fills the mel padding: no row may read past its own frames


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test requires a ROCm device")
    return torch.device("cuda:0")


_cache = {}


def _model(name):
    """(fixture, model) for a fixture name; built once."""
    from tts_amd import GlowTts
    if name not in _cache:
        fx = load_fixture(name)
        enc = str(fx["encoder_type"])
        cfg = GlowConfig(encoder_type=enc, num_speakers=int(fx["num_speakers"]), c_in_channels=int(fx["c_in"]))
        sd = synth_state_dict(glow_spec(cfg), int(fx["seed"]))
        m = GlowTts(num_chars=cfg.num_chars, num_speakers=cfg.num_speakers, c_in_channels=cfg.c_in_channels,
                    encoder_type=enc, use_encoder_prenet=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _cache[name] = (fx, m.to(_dev()).eval())
    return _cache[name]


def _call(m, fx, rows):
    """forward on the fixture rows as one padded batch; the 7 outputs and last_logp as numpy."""
    dev = _dev()
    ids = [fx[f"u{i}_ids"] for i in rows]
    mels = [fx[f"u{i}_mel"] for i in rows]
    T, Ty = max(len(x) for x in ids), max(x.shape[1] for x in mels)
    x = np.zeros((len(rows), T), np.int64)
    y = np.full((len(rows), 80, Ty), PAD, np.float32)
    for b, (i, mel) in enumerate(zip(ids, mels)):
        x[b, :len(i)] = i
        y[b, :, :mel.shape[1]] = mel
    g = torch.tensor([int(fx[f"u{i}_spk"]) for i in rows]) if int(fx["num_speakers"]) > 1 else None
    out = m.forward(torch.from_numpy(x).to(dev), [len(i) for i in ids], torch.from_numpy(y).to(dev),
                    torch.tensor([mel.shape[1] for mel in mels]), g=g)
    return [o.cpu().numpy() for o in out] + [m.last_logp.cpu().numpy()]


def _batched(name):
    """All four rows in one call; computed once per fixture and shared (read-only) by the tests."""
    key = name + ":out"
    if key not in _cache:
        fx, m = _model(name)
        _cache[key] = _call(m, fx, range(len(ROWS)))
    return _cache[key]


@pytest.mark.parametrize("name", ["glow_fwd", "glow_fwd_spk"])
def test_mas_is_exact_on_the_reference_logp(name):
    """tts_glow_mas on the fixture's fp32 logp, all four rows in one ragged batch: the reference's path."""
    from tts_amd import _lib
    fx = load_fixture(name)
    eng = _lib.get_engine(_dev())
    logp = np.full((len(ROWS), 70, 150), 123.0, np.float32)  # outside a row's lengths: never read
    for i, (tx, ty) in enumerate(ROWS):
        logp[i, :tx, :ty // 2 * 2] = fx[f"u{i}_logp"]
    with eng.lock:
        path = eng.glow_mas(torch.from_numpy(logp).to(_dev()), [tx for tx, _ in ROWS],
                            [ty // 2 * 2 for _, ty in ROWS]).cpu().numpy()
    for i, (tx, ty) in enumerate(ROWS):
        want = np.zeros((70, 150), np.float32)
        want[:tx, :ty // 2 * 2] = fx[f"u{i}_attn"].T
        assert np.array_equal(path[i], want), (name, i)


def _maximum_path(value, t_x, t_y):
    """``monotonic_align/core.pyx:9-35`` with the x loop as float32 vector operations (the same one
    max and one add per cell): ``value`` (t_x, t_y) -> path (t_x, t_y)."""
    q = value.astype(np.float32).copy()
    neg = np.float32(-1e9)
    for y in range(t_y):
        lo, hi = max(0, t_x + y - t_y), min(t_x, y + 1)
        xs = np.arange(lo, hi)
        prev_col = q[:, y - 1] if y > 0 else np.zeros(t_x, np.float32)
        v_cur = np.where(xs == y, neg, prev_col[xs])
        v_prev = np.where(xs == 0, np.float32(0) if y == 0 else neg, prev_col[np.maximum(xs - 1, 0)])
        q[lo:hi, y] = np.maximum(v_cur, v_prev).astype(np.float32) + q[lo:hi, y]
    path = np.zeros((t_x, t_y), np.float32)
    index = t_x - 1
    for y in range(t_y - 1, -1, -1):
        path[index, y] = 1
        if index != 0 and (index == y or q[index, y - 1] < q[index - 1, y - 1]):
            index -= 1
    return path


def test_mas_beyond_one_workgroup_of_tokens():
    """More tokens than the search's 1024 threads (several tokens per thread), a forced diagonal of
    1025 and a short row in one ragged batch, on random values, against the restated search (which
    first has to reproduce the fixture's largest row)."""
    from tts_amd import _lib
    fx = load_fixture("glow_fwd")
    assert np.array_equal(_maximum_path(fx["u3_logp"], 70, 150), fx["u3_attn"].T)
    rows = ((1100, 1200), (1025, 1025), (300, 1400))
    Tx, Ty = 1100, 1400
    logp = (np.random.RandomState(11).randn(len(rows), Tx, Ty) * 8 - 100).astype(np.float32)
    eng = _lib.get_engine(_dev())
    with eng.lock:
        path = eng.glow_mas(torch.from_numpy(logp).to(_dev()), [r[0] for r in rows], [r[1] for r in rows]).cpu().numpy()
    for i, (tx, ty) in enumerate(rows):
        want = np.zeros((Tx, Ty), np.float32)
        want[:tx, :ty] = _maximum_path(logp[i, :tx, :ty], tx, ty)
        assert np.array_equal(path[i], want), i


@pytest.mark.parametrize("name", ["glow_fwd", "glow_fwd_spk"])
def test_forward_matches_reference(name):
    fx = load_fixture(name)
    z, logdet, y_mean, y_log_scale, attn, o_dur_log, o_attn_dur, logp = _batched(name)
    Te = 150
    assert z.shape == (4, 80, Te) and logdet.shape == (4,) and y_mean.shape == (4, 80, Te)
    assert attn.shape == (4, Te, 70) and o_dur_log.shape == (4, 1, 70) and o_attn_dur.shape == (4, 1, 70)
    assert logp.shape == (4, 70, Te) and not y_log_scale.any() and y_log_scale.shape == y_mean.shape
    fails = []
    for i, (tx, ty) in enumerate(ROWS):
        k, te = f"u{i}", ty // 2 * 2
        want = np.zeros((Te, 70), np.float32)
        want[:te, :tx] = fx[k + "_attn"]
        assert np.array_equal(attn[i], want), (name, k)
        assert np.abs(o_attn_dur[i, 0, :tx] - fx[k + "_oattn_dur"]).max() <= 1e-6 and not o_attn_dur[i, 0, tx:].any()
        assert np.abs(o_dur_log[i, 0, :tx] - fx[k + "_logw"]).max() <= 1e-5 and not o_dur_log[i, 0, tx:].any()
        assert np.abs(y_mean[i, :, :te] - fx[k + "_ymean"]).max() <= MEL_TOL and not y_mean[i, :, te:].any()
        assert not z[i, :, te:].any() and not logp[i, tx:].any() and not logp[i, :, te:].any()
        errs = {"z": np.abs(z[i, :, :te] - fx[k + "_z64"]).max(),
                "logp": np.abs(logp[i, :tx, :te] - fx[k + "_logp64"]).max(),
                "logdet": abs(float(logdet[i]) - float(fx[k + "_logdet64"]))}
        for q, err in errs.items():
            bound = FACTOR * float(fx[f"{k}_{q}_drift"])
            if q == "z":
                bound = max(bound, MEL_TOL)
            print(f"{name} {k} {q}: err {err:.3e} bound {bound:.3e} (reference fp32 drift {float(fx[f'{k}_{q}_drift']):.3e})")
            if not err <= bound:
                fails.append((k, q, float(err), bound))
    assert not fails, fails


def test_row_alone_equals_its_slice_of_the_batch():
    """Row (5, 11) alone is bit for bit its slice of the batched call."""
    fx, m = _model("glow_fwd")
    full = _batched("glow_fwd")
    z, logdet, y_mean, _, attn, o_dur_log, o_attn_dur, logp = _call(m, fx, [1])
    assert z.shape == (1, 80, 10) and attn.shape == (1, 10, 5)
    assert np.array_equal(z[0], full[0][1, :, :10]) and logdet[0] == full[1][1]
    assert np.array_equal(y_mean[0], full[2][1, :, :10]) and np.array_equal(attn[0], full[4][1, :10, :5])
    assert np.array_equal(o_dur_log[0], full[5][1, :, :5]) and np.array_equal(o_attn_dur[0], full[6][1, :, :5])
    assert np.array_equal(logp[0], full[7][1, :5, :10])


def test_forward_on_its_own_noise_free_mel():
    """forward(x, y = inference(x, noise = 0).y) on the glow fixture's u1: the durations the reference's
    forward finds on its own noise-free mel (``rt_dur``; the row meets the margin condition). They
    equal inference's w_ceil only where no token has a zero duration, which the fixture records as
    ``rt_ok`` (0 for u1: 18 of its 31 tokens get no frame from generate_path)."""
    fx, m = _model("glow_fwd")
    ids = load_fixture("glow")["u1_ids"]
    x = torch.from_numpy(ids[None]).to(_dev())
    y, _, _, _, attn_inf, _, _ = m.inference(x, [len(ids)], noise=torch.zeros(1, 80, 4096, device=_dev()))
    w_ceil = attn_inf[0].sum(0).cpu().numpy()
    assert np.array_equal(w_ceil, fx["rt_w_ceil"]) and y.shape[2] == int(w_ceil.sum())
    o_attn_dur = m.forward(x, [len(ids)], y)[6]
    dur = np.rint(np.exp(o_attn_dur[0, 0].cpu().numpy()) - 1)
    assert np.array_equal(dur, fx["rt_dur"])
    if int(fx["rt_ok"]):
        assert np.array_equal(dur, w_ceil)


def test_errors():
    fx, m = _model("glow_fwd")
    dev = _dev()
    x = torch.ones(2, 6, dtype=torch.long, device=dev)
    y = torch.zeros(2, 80, 12, device=dev)
    with pytest.raises(ValueError, match="row 1"):  # 5 -> 4 even frames for 6 tokens
        m.forward(x, [6, 6], y, torch.tensor([12, 5]))
    with pytest.raises(ValueError, match="row 0"):  # fewer than 2 frames
        m.forward(x, [1, 6], y, torch.tensor([1, 12]))
    with pytest.raises(ValueError, match="y_lengths"):
        m.forward(x, [6, 6], y, torch.tensor([12, 13]))
    with pytest.raises(AttributeError, match="size"):
        m.forward(x, [6, 6])
    with pytest.raises(AttributeError, match="emb_g"):
        m.forward(x, [6, 6], y, g=torch.tensor([0, 0]))
    _, ms = _model("glow_fwd_spk")
    with pytest.raises(RuntimeError, match="pass g"):
        ms.forward(x, [6, 6], y)
    with pytest.raises(IndexError):
        ms.forward(x, [6, 6], y, g=torch.tensor([0, 3]))
    # the C entry point refuses the same rows with a message that names the row
    from tts_amd import _lib
    eng = _lib.get_engine(dev)
    with eng.lock, pytest.raises(RuntimeError, match="row 1 has fewer frames than tokens"):
        eng.glow_mas(torch.zeros(2, 6, 12, device=dev), [6, 6], [12, 5])
