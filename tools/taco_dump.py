"""Tacotron2 outputs (bench.py's random-init C2 model, the first 12 LJ-profile utterances, forced
lengths at r = 2) saved to an .npz file, for bit-identity checks between library settings run in
separate processes (e.g. TTS_BAR_CALIBRATE=0 / 1: the decoder's barrier blocks picked by timing or
taken in order; the barrier's place must not change a single bit).

    python tools/taco_dump.py out.npz [n]     (n utterances, default 12; > 32 repeats the profile)
    python tools/taco_dump.py out.npz golden  (the taco_sigmoid fixture's three r = 2 utterances, built
                                               as tests/test_gpu_parity.py's batched test builds them)
    python tools/taco_dump.py out.npz stops   (the taco_stops fixture's 17-row r = 2 batch in its stored
                                               caller order: rows that stop by the stopnet, max steps 32)
    python tools/taco_dump.py out.npz teacher (the taco_teacher fixture's four r = 2 rows as one batch
                                               through the teacher-forced forward; no steps / status)

Every file also holds `path`, the decoder path of the call (Engine.decoder_stats(): 1 persistent,
0 captured step graphs), and `status` (per row, 1 = stopnet, 2 = max_decoder_steps).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tts_amd._lib import get_engine  # noqa: E402


def bench_run(dev, n):
    import bench
    from tts_amd.workload import forced_steps, lj_profile, pad_batch, synthetic_ids
    taco, _, _, _, _, _ = bench.build_models(dev)
    taco.decoder.verbose = False
    taco.decoder.set_r(2)
    T, M = lj_profile()
    T, M = (list(T) * 2)[:n], (list(M) * 2)[:n]
    batch, lens = pad_batch(synthetic_ids(T))
    return taco, taco.inference(torch.from_numpy(batch).to(dev), text_lengths=lens,
                                max_decoder_steps=forced_steps(M, 2))


def golden_run(dev, r=2):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import build_taco, load_fixture, taco_state_dict
    fx = load_fixture("taco_sigmoid")
    cfg, sd = taco_state_dict(fx, r=r)
    m = build_taco(cfg, sd, dev)
    m.decoder.set_r(r)
    m.decoder.max_decoder_steps = int(fx[f"r{r}_max_steps"])
    ids = [fx[f"r{r}_u{i}_ids"] for i in range(3)]
    T = max(len(x) for x in ids)
    batch = np.zeros((3, T), np.int64)
    for i, x in enumerate(ids):
        batch[i, :len(x)] = x
    return m, m.inference(torch.from_numpy(batch).to(dev), text_lengths=[len(x) for x in ids])


def stops_run(dev, r=2, B=17):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import build_taco, load_fixture, stop_batch, stop_model
    fx = load_fixture("taco_stops")
    cfg, sd = stop_model(fx, f"r{r}")
    m = build_taco(cfg, sd, dev)
    m.decoder.set_r(r)
    m.decoder.max_decoder_steps = int(fx[f"r{r}_max_steps"])
    m.decoder.verbose = False
    batch, lens, _, _, _ = stop_batch(fx, r, fx[f"r{r}_order{B}"])
    return m, m.inference(torch.from_numpy(batch).to(dev), text_lengths=lens)


def teacher_run(dev, r=2):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import build_taco, load_fixture, taco_state_dict
    fx = load_fixture("taco_teacher")
    cfg, sd = taco_state_dict(fx, r=r)
    m = build_taco(cfg, sd, dev)
    m.decoder.set_r(r)
    m.decoder.verbose = False
    ids = [fx[f"r{r}_u{u}_ids"] for u in range(4)]
    mels = [fx[f"r{r}_u{u}_mel"] for u in range(4)]
    T, M = max(len(i) for i in ids), max(-(-len(x) // r) * r for x in mels)
    text, mel = np.zeros((4, T), np.int64), np.full((4, M, 80), 1e3, np.float32)  # no row may read its padding
    for b, (i, x) in enumerate(zip(ids, mels)):
        text[b, :len(i)], mel[b, :len(x)] = i, x
    return m.forward(torch.from_numpy(text).to(dev), torch.tensor([len(i) for i in ids]),
                     torch.from_numpy(mel).to(dev), torch.tensor([len(x) for x in mels]))


def main(path, mode="12"):
    dev = torch.device("cuda", 0)
    if mode == "teacher":
        dec, post, align, stop = teacher_run(dev)
        return np.savez(path, dec=dec.cpu().numpy(), post=post.cpu().numpy(), align=align.cpu().numpy(),
                        stop=stop.cpu().numpy(), path=np.asarray(get_engine("cuda:0").decoder_stats()[0]))
    taco, (dec, post, align, stop) = (golden_run(dev) if mode == "golden" else stops_run(dev) if mode == "stops"
                                        else bench_run(dev, int(mode)))
    np.savez(path, dec=dec.cpu().numpy(), post=post.cpu().numpy(), align=align.cpu().numpy(),
             stop=stop.cpu().numpy(), steps=np.asarray(taco.last_steps), status=np.asarray(taco.last_status),
             path=np.asarray(get_engine("cuda:0").decoder_stats()[0]))


if __name__ == "__main__":
    main(*sys.argv[1:3])
