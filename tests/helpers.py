"""Shared fixture plumbing for the parity tests (weights are regenerated from seeds)."""
import json
import math
import os

import numpy as np
import torch

from tts_amd.spec import MelganConfig, TacotronConfig, melgan_layers, melgan_spec, tacotron2_spec
from tts_amd.weights import synth_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def taco_cfg(fx):
    return TacotronConfig(**json.loads(str(fx["cfg"])))


def taco_state_dict(fx, r=None, seed=None, overrides=None, stop_bias=None, cfg=None):
    cfg = cfg or taco_cfg(fx)
    if seed is None:  # per-r seed when the fixture's stop-margin search moved it between r values
        seed = int(fx[f"r{r}_seed"]) if r is not None and f"r{r}_seed" in fx.files else int(fx["seed"])
    ov = json.loads(str(fx["overrides"])) if overrides is None else overrides
    sd = synth_state_dict(tacotron2_spec(cfg), seed, ov)
    if stop_bias is None and r is not None:
        stop_bias = float(fx[f"r{r}_stop_bias"])
    if stop_bias is not None:
        sd["decoder.stopnet.1.linear_layer.bias"] = np.array([stop_bias], np.float32)
    return cfg, sd


def build_taco(cfg, sd, device="cuda"):
    from tts_amd import Tacotron2
    m = Tacotron2(num_chars=cfg.num_chars, num_speakers=cfg.num_speakers, r=cfg.r, attn_norm=cfg.attn_norm,
                  double_decoder_consistency=cfg.double_decoder_consistency, ddc_r=cfg.ddc_r,
                  speaker_embedding_dim=cfg.speaker_embedding_dim, prenet_type=cfg.prenet_type,
                  attn_win=cfg.windowing, forward_attn=cfg.forward_attn, trans_agent=cfg.trans_agent,
                  forward_attn_mask=cfg.forward_attn_mask, attn_type=cfg.attn_type, attn_K=cfg.attn_K,
                  bidirectional_decoder=cfg.bidirectional_decoder)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(device).eval()


# ---- taco_stops.npz: batches with stopnet-driven stops (tests/golden/make_stop_golden.py) ----
STOP_MARGIN = 1e-2           # min |logit + bias| up to a row's stop (make_golden.py's margin)
STOP_DRIFT_MAX = 1e-4 / 8    # the reference's own fp32-vs-fp64 postnet difference: MEL_TOL / 8
STOP_SHRINK_BY = 8           # shrink-early order: the last batch tile's rows all stop by this step
STOP_BATCHES = (17, 36, 64)  # the batches are rows 0..B-1 of a group, in the stored caller orders


def decode_order(lens):
    """The library's decode order for equal max_decoder_steps: stable sort by text length, descending
    (api_taco.hip stage_decode_order, a step of taco_run); decode row i = caller row decode_order(lens)[i]."""
    return np.argsort(-np.asarray(lens, np.int64), kind="stable")


def stop_steps_from_logits(z, max_steps, steps=None):
    """The reference's stop rule on biased logits z (n, max_steps): stop at the first t > 0 with z_t > 0
    (sigmoid > 0.5), else at max_steps. Returns (steps, status 1 = stopnet / 2 = max steps, margin =
    min |z_t| over the deciding steps 1..stop). `steps`: rows of z hold only that many logits."""
    z = np.asarray(z, np.float64)
    n = len(z)
    out_steps, status, margin = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
    for i in range(n):
        zi = z[i, :max_steps if steps is None else int(steps[i])]
        hit = np.nonzero(zi[1:] > 0)[0]
        out_steps[i] = hit[0] + 2 if len(hit) else len(zi)
        status[i] = 1 if len(hit) else 2
        margin[i] = np.abs(zi[1:out_steps[i]]).min() if out_steps[i] > 1 else np.inf
    return out_steps, status, margin


def stop_spread_problems(lens, steps, status, max_steps, shrink_by=None):
    """The spread conditions on one batch in caller order that are violated (none: an empty list).
    Tiles are the decoder's 16-row batch tiles in decode order. With `shrink_by` the two conditions on
    the last tile (it outlives a tile-0 stopper; it holds a max-steps row) are replaced: it must hold
    only rows that stop by that step, while lower tiles hold both a row already frozen by then and a
    live one."""
    lens, steps, status = np.asarray(lens), np.asarray(steps), np.asarray(status)
    B = len(lens)
    o = decode_order(lens)
    s, st = steps[o], status[o]
    tiles = [slice(a, min(a + 16, B)) for a in range(0, B, 16)]
    bad = []
    if len(set(s.tolist())) < 6:
        bad.append("fewer than 6 distinct step counts")
    if 4 * int((st == 1).sum()) < B:
        bad.append("fewer than a quarter of the rows stop by the stopnet")
    if int((st == 2).sum()) < max(2, B // 10):
        bad.append("too few rows run to max_decoder_steps")
    if ((st == 2) & (s != max_steps)).any():
        bad.append("a status-2 row below max_decoder_steps")
    for k, t in enumerate(tiles):
        if t.stop - t.start > 1 and not any(st[i] == 1 and (s[t] > s[i]).any() for i in range(t.start, t.stop)):
            bad.append(f"tile {k}: no stopnet-stopped row beside a row that finishes later")
    last = tiles[-1]
    if shrink_by is None:
        if len(tiles) > 1 and not ((st[tiles[0]] == 1) & (s[tiles[0]] < s[last].max())).any():
            bad.append("no tile-0 row stops before the last tile finishes")
        if not (st[last] == 2).any():
            bad.append("the last tile holds no row that runs to max_decoder_steps")
    else:
        below = s[:last.start]
        if not (s[last] <= shrink_by).all():
            bad.append(f"a last-tile row runs past step {shrink_by}")
        if not ((below <= s[last].max()).any() and (below > s[last].max()).any()):
            bad.append("no frozen row beside a live one below the last tile when it falls away")
    return bad


def stop_tags(fx):
    return [t for t in ("r2", "r1", "spk") if t + "_steps" in fx.files]


def stop_fixture_problems(fx, tags=None):
    """Every condition make_stop_golden.py asserts on its selection, re-derived from the stored data
    alone (conditions on the reference, not on the code under test); the violated ones."""
    bad = []
    for tag in tags or stop_tags(fx):
        p = tag + "_"
        S = int(fx[p + "max_steps"])
        lens, steps = fx[p + "lens"], fx[p + "steps"]
        st, status, margin = stop_steps_from_logits(fx[p + "logits"], S, steps)
        if not np.array_equal(st, steps):
            bad.append(f"{tag}: the stored logits do not give the stored step counts")
        if margin.min() < STOP_MARGIN:
            bad.append(f"{tag}: stop margin {margin.min():.3e}")
        if not np.array_equal(fx[p + "steps64"], steps):
            bad.append(f"{tag}: the fp64 run stops elsewhere")
        if fx[p + "drift64"].max() > STOP_DRIFT_MAX:
            bad.append(f"{tag}: drift64 {fx[p + 'drift64'].max():.2e}")
        if lens.min() < 1 or lens.max() > 30 or (len(lens) == 64 and ((lens == 1).sum() < 2 or len(set(lens.tolist())) < 12 or lens.max() < 25)):
            bad.append(f"{tag}: text lengths not mixed over 1..30 with two rows of length 1")
        orders = [f"order{n}" for n in STOP_BATCHES if n <= len(lens)] + (["order36_shrink"] if len(lens) >= 36 else [])
        for name in orders:
            o = fx[p + name]
            n = int(name[5:7])
            if sorted(o.tolist()) != list(range(n)):
                bad.append(f"{tag} {name}: not an order of rows 0..{n - 1}")
                continue
            for msg in stop_spread_problems(lens[o], steps[o], status[o], S, STOP_SHRINK_BY if "shrink" in name else None):
                bad.append(f"{tag} {name}: {msg}")
    return bad


def stop_model(fx, tag):
    """(cfg, state dict) of a taco_stops group: the seeded model with its recorded gains and stop bias."""
    cfg = TacotronConfig(**json.loads(str(fx[tag + "_cfg"])))
    return taco_state_dict(None, seed=int(fx[tag + "_seed"]), overrides=json.loads(str(fx[tag + "_gains"])),
                           stop_bias=float(fx[tag + "_stop_bias"]), cfg=cfg)


def stop_batch(fx, r, rows, tag=None):
    """Rows `rows` (caller order) of the taco_stops group `tag` (default f"r{r}") as one padded batch:
    (ids (B, T_max) int64, text lengths, the reference's step counts, statuses, speaker ids or None).
    Checks in numpy that these rows' stored stop logits keep the stop margin."""
    tag = tag or f"r{r}"
    p = tag + "_"
    assert int(fx[p + "r"]) == r
    rows = np.asarray(rows)
    lens = fx[p + "lens"][rows]
    steps, status, margin = stop_steps_from_logits(fx[p + "logits"][rows], int(fx[p + "max_steps"]), fx[p + "steps"][rows])
    assert np.array_equal(steps, fx[p + "steps"][rows]) and margin.min() >= STOP_MARGIN, "stop_margin"
    batch = np.zeros((len(rows), int(lens.max())), np.int64)
    for k, i in enumerate(rows):
        batch[k, :lens[k]] = fx[p + "ids"][i, :lens[k]]
    spk = fx[p + "spk"][rows] if p + "spk" in fx.files else None
    return batch, [int(x) for x in lens], steps, status, spk


# ---- Tacotron (v1): the stop bias of a batch (tests/golden/make_tacotron1_golden.py) ----
L06 = math.log(0.6 / 0.4)    # the stop rule's threshold sigmoid(logit) > 0.6, as a logit


def choose_bias(raw, Ts, aligns, max_steps, min_token_stops, need_max_row, min_stop_step=3):
    """Stop bias with the widest margin |l_t + b - logit(0.6)| over the tested steps (t > T/4, up to
    each row's stop), such that at least min_token_stops rows stop by the token (not before
    min_stop_step) and, if asked, a row runs max_steps + 1 steps."""
    elig = [np.arange(len(l)) + 1 > T / 4 for l, T in zip(raw, Ts)]
    cands = np.sort(np.concatenate([L06 - l[e] for l, e in zip(raw, elig)]))
    best = None
    for b in (cands[:-1] + cands[1:]) / 2:
        margins, ntok, nmax, ok = [], 0, 0, True
        for l, e, a, T in zip(raw, elig, aligns, Ts):
            z = l + b - L06
            by_align = e & (a[:len(l), T - 1] > 0.6)
            idx_tok = np.nonzero(e & (z > 0))[0]
            idx_al = np.nonzero(by_align)[0]
            s_tok = idx_tok[0] if len(idx_tok) else len(l)
            s_al = idx_al[0] if len(idx_al) else len(l)
            end = min(s_tok, s_al, len(l) - 1)
            if s_tok < s_al:
                ntok += 1
                ok &= s_tok + 1 >= min_stop_step
            elif s_al == len(l) and len(l) == max_steps + 1:
                nmax += 1
            tested = e[:end + 1]
            if tested.any():
                margins.append(np.abs(z[:end + 1][tested]).min())
        if not ok or ntok < min_token_stops or (need_max_row and nmax < 1):
            continue
        mm = min(margins)
        if best is None or mm > best[1]:
            best = (float(b), float(mm), ntok, nmax)
    return best


# ---- tacotron1_f64.npz: float64 arrays as fixed point in byte planes, so that they compress ----
F64_BITS = 38  # stored values are multiples of 2^-38 (|x| < 2^25)


def pack_f64(x):
    """x (float64, any shape) -> uint8 (8, *x.shape): byte planes of round(x * 2^38) as little-endian int64."""
    q = np.round(np.asarray(x, np.float64) * 2.0 ** F64_BITS).astype("<i8")
    return np.ascontiguousarray(np.moveaxis(q[..., None].view(np.uint8), -1, 0))


def unpack_f64(planes):
    q = np.ascontiguousarray(np.moveaxis(np.asarray(planes, np.uint8), 0, -1)).view("<i8")[..., 0]
    return q.astype(np.float64) / 2.0 ** F64_BITS


_t1 = {}


def taco1_f64():
    """tacotron1_f64.npz, loaded once: (arrays by key, the new cases by tag)."""
    if "f64" not in _t1:
        fx = np.load(os.path.join(GOLDEN, "tacotron1_f64.npz"))
        _t1["f64"] = (fx, {c["tag"]: c for c in json.loads(str(fx["cases"]))})
    return _t1["f64"]


def taco1_state_dict(cfg, seed, gains, stop_bias):
    from tts_amd.spec import tacotron_spec
    sd = synth_state_dict(tacotron_spec(cfg), seed, gains)
    sd["decoder.stopnet.linear.bias"] = np.array([stop_bias], np.float32)
    return sd


def taco1_case(tag, **cfg_changes):
    """(cfg, state dict, case record) of a new case of tacotron1_f64.npz; cfg_changes: e.g. another
    postnet_output_dim on the same seed."""
    from tts_amd.spec import TacotronV1Config
    fx, cases = taco1_f64()
    c = cases[tag]
    cfg = TacotronV1Config(**dict(c["cfg"], **cfg_changes))
    return cfg, taco1_state_dict(cfg, c["seed"], json.loads(str(fx["overrides"])), c["stop_bias"]), c


def taco1_oracles(cfg, sd, hook=None):
    """The float64 oracle and its float32 evaluation (the yardstick e32)."""
    from oracle.tacotron1_np import Tacotron1Oracle
    return Tacotron1Oracle(sd, cfg, hook=hook), Tacotron1Oracle(sd, cfg, np.float32)


def build_taco1(cfg, sd, device="cuda"):
    from tts_amd import Tacotron
    m = Tacotron(num_chars=cfg.num_chars, num_speakers=0, r=cfg.r, postnet_output_dim=cfg.postnet_output_dim,
                 attn_norm=cfg.attn_norm, memory_size=cfg.memory_size)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(device).eval()


def melgan_state_dict(seed, cfg=None):
    cfg = cfg or MelganConfig()
    return cfg, synth_state_dict(melgan_spec(cfg, weight_norm=True), seed)


def build_melgan(cfg, sd, device="cuda"):
    from tts_amd import MultibandMelganGenerator
    v = MultibandMelganGenerator(in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                                 base_channels=cfg.base_channels, upsample_factors=cfg.upsample_factors,
                                 num_res_blocks=cfg.num_res_blocks)
    full = v.state_dict()
    for k, t in sd.items():
        full[k] = torch.from_numpy(t)
    v.load_state_dict(full)
    v.remove_weight_norm()
    return v.to(device).eval()


def melgan_oracle(cfg, sd):
    from oracle.melgan_np import MelganOracle
    from tts_amd.pqmf import pqmf_filters
    return MelganOracle(sd, melgan_layers(cfg), pqmf_filters()[1])
