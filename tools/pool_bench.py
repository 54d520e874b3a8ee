"""A/B of `functional.pooled_layer_norm` (the fused LayerNorm + pool kernels, csrc/pool_rows.hip) against the same head composed from what
the package offered before it: `functional.layer_norm` (one launch that writes the normalised [B, T, D] tensor), then torch's `mean(1)`, or
a matrix product with the projection, `softmax(dim=1)`, a transpose and a batched matrix product.  Both run in one process, alternating, on
the same parameters and inputs; device events around windows of `--iters` calls; the median of `--windows` windows is reported with the
spread, and the outputs of the two paths are compared first.  Shapes: the ViT-B/16 stream (B 128, T 196, D 768) and a long sequence
(B 8, T 4096, D 256), f32 rows, both poolers.  Also the fused forward's bytes per second against its minimum traffic (one read of x).

    python tools/pool_bench.py [--out profiles/r18/pool_ab.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cflearn_amd import functional as HF  # noqa: E402

SHAPES = [(128, 196, 768), (8, 4096, 256)]  # B, T, D
EPS = 1e-6


def composed(x, gamma, beta, pool, w, b):
    """the parent's parts, the reference's op order (poolers.py:33-39 / api.py:382)"""
    y = HF.layer_norm(x, gamma, beta, EPS, out_f32=True)
    if pool == "mean":
        return y.mean(1)
    weights = torch.softmax(y @ w.t() + b, dim=1).transpose(-1, -2)
    return torch.matmul(weights, y).squeeze(-2)


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def ab(fa, fb, iters, windows):
    for fn in (fa, fb):
        for _ in range(3):
            fn()
    ta, tb = [], []
    for _ in range(windows):  # alternate
        ta.append(window(fa, iters))
        tb.append(window(fb, iters))
    return ta, tb


def fmt(ts):
    return f"{statistics.median(ts):8.4f} ms (min {min(ts):.4f}, max {max(ts):.4f})"


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " | ".join(l.strip() for l in out.splitlines() if "sclk" in l or "mclk" in l)[:400] or "not reported"
    except Exception as e:  # the tool is not installed / not permitted: say so, do not guess
        return f"not read ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "pool_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pool_bench needs the MI355X"
    dev = "cuda:0"
    lines = [f"pool_bench: {torch.cuda.get_device_name(0)}; clocks before: {clocks()}",
             f"{args.windows} windows of {args.iters} calls per path, alternating; median (min, max) per call"]
    for bsz, t, d in SHAPES:
        torch.manual_seed(0)
        x = torch.randn(bsz, t, d, device=dev)
        dout = torch.randn(bsz, d, device=dev)
        gamma = torch.nn.Parameter(1.0 + 0.1 * torch.randn(d, device=dev))
        beta = torch.nn.Parameter(0.1 * torch.randn(d, device=dev))
        w = torch.nn.Parameter(torch.randn(1, d, device=dev) * d ** -0.5)
        b = torch.nn.Parameter(torch.zeros(1, device=dev))
        for pool in ("mean", "sequence"):
            extra = (w, b) if pool == "sequence" else ()
            fa = lambda v: HF.pooled_layer_norm(v, gamma, beta, EPS, pool, *extra)  # noqa: E731
            fb = lambda v: composed(v, gamma, beta, pool, w, b)  # noqa: E731
            with torch.no_grad():
                ya, yb = fa(x), fb(x)
            lines.append(f"\nB {bsz}, T {t}, D {d}, {pool}: outputs rel-L2 fused vs composed {((ya - yb).norm() / yb.norm()).item():.2e}")

            def fwd(f):
                with torch.no_grad():
                    f(x)

            def fwd_bwd(f):
                for p in (gamma, beta, w, b):
                    p.grad = None
                xg = x.detach().requires_grad_()
                f(xg).backward(dout)

            for name, run in (("forward", fwd), ("forward + backward", fwd_bwd)):
                ta, tb = ab(lambda: run(fa), lambda: run(fb), args.iters, args.windows)
                lines.append(f"  {name:18s} fused {fmt(ta)}   composed {fmt(tb)}   composed / fused {statistics.median(tb) / statistics.median(ta):.2f}")
                if name == "forward":
                    nbytes = bsz * t * d * 4
                    lines.append(f"  {'':18s} fused forward: minimum traffic {nbytes / 1e6:.1f} MB -> {nbytes / statistics.median(ta) / 1e6:.0f} GB/s")
    lines.append(f"\nclocks after: {clocks()}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
