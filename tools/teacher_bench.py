"""Teacher-forced Tacotron2.forward on the C2 lengths (32 utterances, lj_profile lengths, r = 2).

Synthetic weights and ids as bench.py's workload; the teacher mel is the model's own free-running
postnet output at the forced LJ lengths. Prints one JSON line: ms per forward call, us per decoder
step (the whole call over the longest row's steps; it includes the encoder, the teacher prenet GEMM
and the postnet) and, for scale, the free-running inference() call on the same rows. No threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tts_amd import Tacotron2  # noqa: E402
from tts_amd.spec import TacotronConfig, tacotron2_spec  # noqa: E402
from tts_amd.weights import synth_state_dict  # noqa: E402
from tts_amd.workload import forced_steps, lj_profile, pad_batch, synthetic_ids  # noqa: E402


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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--r", type=int, default=2)
    a = ap.parse_args()
    T, M = lj_profile()
    T = [T[i % len(T)] for i in range(a.batch)]
    M = [M[i % len(M)] for i in range(a.batch)]
    cfg = TacotronConfig()
    m = Tacotron2(num_chars=cfg.num_chars, r=cfg.r, attn_norm=cfg.attn_norm, double_decoder_consistency=True,
                  ddc_r=cfg.ddc_r)
    sd = synth_state_dict(tacotron2_spec(cfg), 1)
    sd["decoder.stopnet.1.linear_layer.bias"] = np.array([-1e4], np.float32)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    m.decoder.set_r(a.r)
    m.decoder.verbose = False
    batch, lens = pad_batch(synthetic_ids(T))
    x = torch.from_numpy(batch).cuda()
    ms = np.array(forced_steps(M, a.r))
    mel = m.inference(x, text_lengths=lens, max_decoder_steps=ms)[1].contiguous()  # (B, max S r, 80)
    mlens = torch.tensor(M)
    t_fwd = timed(lambda: m.forward(x, lens, mel, mlens), a.steps, a.warmup)
    assert list(m.last_steps) == list(ms)
    t_inf = timed(lambda: m.inference(x, text_lengths=lens, max_decoder_steps=ms), a.steps, a.warmup)
    S = int(ms.max())
    print(json.dumps({"metric": "tacotron2_forward_ms_per_call", "value": t_fwd * 1e3, "us_per_step": t_fwd / S * 1e6,
                      "inference_ms_per_call": t_inf * 1e3, "inference_us_per_step": t_inf / S * 1e6,
                      "decoder_steps_max": S, "decoder_steps_sum": int(ms.sum()), "frames": int(sum(M)),
                      "chars": int(sum(T)), "batch": a.batch, "r": a.r}))


if __name__ == "__main__":
    main()
