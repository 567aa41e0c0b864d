"""Tacotron (v1) inference throughput on the LJSpeech-shaped batch (32 utterances, lj_profile lengths).

Synthetic weights (tts_amd.weights) and ids, r = 5, postnet_output_dim 1025. Random weights never
raise the stop token, so each row's length is forced by its own max_decoder_steps: a row that never
stops runs max_decoder_steps + 1 steps, which is set to ceil(M / r) of the LJ profile. Prints one
JSON line: ms per call, us per decoder step (the call minus the encoder and postnet stages, over the
longest row's steps) and mel frames/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tts_amd import Tacotron  # noqa: E402
from tts_amd.spec import TacotronV1Config, tacotron_spec  # noqa: E402
from tts_amd.weights import synth_state_dict  # noqa: E402
from tts_amd.workload import lj_profile, pad_batch, synthetic_ids  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    T, M = lj_profile()
    T = [T[i % len(T)] for i in range(a.batch)]
    M = [M[i % len(M)] for i in range(a.batch)]
    cfg = TacotronV1Config()
    r = cfg.r
    m = Tacotron(num_chars=cfg.num_chars, num_speakers=0, r=r, postnet_output_dim=cfg.postnet_output_dim,
                 memory_size=cfg.memory_size)
    sd = synth_state_dict(tacotron_spec(cfg), 3)
    sd["decoder.stopnet.linear.bias"] = np.array([-1e4], np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    m.decoder.verbose = False
    batch, lens = pad_batch(synthetic_ids(T))
    x = torch.from_numpy(batch).cuda()
    ms = np.array([max(1, -(-n // r) - 1) for n in M])
    out = {}

    def call():
        out["o"] = m.inference(x, text_lengths=lens, max_decoder_steps=ms)

    dt = timed(call, a.steps, a.warmup)
    steps = m.last_steps.copy()
    frames = int(m.last_mel_lengths.sum())
    dec = out["o"][0]
    t_enc = timed(lambda: m.encode(x, lens), a.steps, a.warmup)
    t_post = timed(lambda: m.run_postnet(dec, m.last_mel_lengths), a.steps, a.warmup)
    S = int(steps.max())
    print(json.dumps({"metric": "tacotron1_mel_frames_per_sec", "value": frames / dt, "ms_per_call": dt * 1e3,
                      "us_per_decoder_step": (dt - t_enc - t_post) / S * 1e6, "encoder_ms": t_enc * 1e3,
                      "postnet_ms": t_post * 1e3, "decoder_steps_max": S, "decoder_steps_sum": int(steps.sum()),
                      "rows_at_forced_length": int((steps == ms + 1).sum()), "frames": frames, "chars": int(sum(T)),
                      "batch": a.batch, "r": r, "postnet_output_dim": cfg.postnet_output_dim}))


if __name__ == "__main__":
    main()
