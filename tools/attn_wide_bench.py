"""The wide-head attention forward (csrc/attn_wide.hip) timed alone on the latent grids of the KL autoencoder's bottleneck:
python tools/attn_wide_bench.py [head_dim] [batch,...]   (T = 1 024 and 4 096 tokens: 256^2 and 512^2 images, one head)

Device events around a window of at least 0.3 s after a warm-up, three windows per shape (the spread is printed).  The roofline
figures are computed from the shapes: 4 B Tq Tk dh FLOP; bytes = Q and O once, K and V once per 128-row query workgroup."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cflearn_amd import ops  # noqa: E402

DH = int(sys.argv[1]) if len(sys.argv) > 1 else 512
BATCHES = [int(b) for b in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 8]
dev = torch.device("cuda")


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us per call


for t in (1024, 4096):
    for b in BATCHES:
        g = torch.Generator(device=dev).manual_seed(t + b)
        q, k, v = ((torch.randn(b, t, DH, device=dev, generator=g) * 0.5).bfloat16() for _ in range(3))
        o = torch.empty_like(q)
        fn = lambda: ops.attn_wide_fwd(q, k, v, 1, head_dim=DH, out=o, want_lse=False)  # noqa: E731
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        reps = max(20, int(0.3e6 / max(window(fn, 10), 1.0)))
        us = sorted(window(fn, reps) for _ in range(3))
        flop = 4.0 * b * t * t * DH
        nbytes = b * (2 * t * DH * 2 + -(-t // 128) * 2 * t * DH * 2)
        print(json.dumps(dict(head_dim=DH, B=b, T=t, reps=reps, us_min=round(us[0], 1), us_median=round(us[1], 1), us_max=round(us[2], 1),
                              tflops=round(flop / us[1] / 1e6, 1), l2_tb_per_s=round(nbytes / us[1] / 1e6, 2))), flush=True)
