"""Time ``tts_taco_style_mel`` (the GST reference encoder + style-token attention, gst.hip) for 32 rows x
800 frames on the weights of the two GST fixtures: ``python tools/gst_bench.py`` on an MI355X. Events
around 20 calls, 5 repeats, after 3 warm-up calls; recorded in profiles/gst/style_mel_time.txt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gst_helpers import build_gst_taco, gst_fixture, gst_state_dict  # noqa: E402


def main(B=32, N=800, calls=20, repeats=5):
    dev = torch.device("cuda:0")
    for tag in ("ext", "tab"):
        fx, cfg = gst_fixture(tag)
        m = build_gst_taco(cfg, gst_state_dict(fx, cfg), dev)
        rs = np.random.RandomState(0)
        mel = torch.from_numpy(rs.randn(B, N, 80).astype(np.float32)).to(dev)
        emb = torch.from_numpy(rs.randn(B, 256).astype(np.float32)).to(dev) if cfg.gst_query_speaker_dim else None
        ragged = np.full(B, N, np.int64)
        ragged[1::2] = 3 * N // 4
        m.style_embedding(mel, style_lengths=ragged, speaker_embeddings=emb)  # loads the weights
        eng = m._engine()
        st = torch.empty(B, cfg.gst_embedding_dim, device=dev)
        for what, lens in ((f"all {N} frames", np.full(B, N)), (f"half of the rows {3 * N // 4} frames", ragged)):
            for _ in range(3):
                eng.taco_style_mel(mel, lens, emb, st)
            torch.cuda.synchronize()
            ts = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    eng.taco_style_mel(mel, lens, emb, st)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) / calls)
            print(f"tts_taco_style_mel {tag} (G={cfg.gst_embedding_dim}) B={B} N={N}, {what}: median "
                  f"{np.median(ts):.3f} ms per call ({repeats} x {calls} calls: min {min(ts):.3f} max {max(ts):.3f})",
                  flush=True)


if __name__ == "__main__":
    main()
