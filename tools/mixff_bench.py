"""A/B of `modules.MixFeedForward` (the depthwise-3x3 + GELU rows kernel, csrc/conv_dw_rows.hip) against the same module composed from what
the package offered before it: Linear, `DepthWiseConv2d` on NCHW (to / from token rows through `HF.tokens_to_nchw` / `HF.nchw_to_tokens`),
`HF.gelu`, Linear.  Both run in one process, alternating, on the same parameters and inputs; device events around windows of `--iters`
calls; the median of `--windows` windows is reported with the spread, and the outputs of the two paths are compared first.  Shapes: the
Mix-Transformer b2 stages at 512 x 512 with the widest and the narrowest token grid that use a 4x expansion.  Also the two convolution
launches alone, with bytes per second against their minimum traffic (forward: read x, write y; backward: read x and dy, write dx).

    python tools/mixff_bench.py [--out profiles/r17/mixff_ab.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cflearn_amd import functional as HF, modules as M, ops  # noqa: E402

SHAPES = [(8, 128, 128, 64, 256), (8, 32, 32, 320, 1280)]  # B, H, W, in_dim, latent_dim


def composed(mod, x, hw):
    """the parent's parts, the reference's op order"""
    h = mod.net[0](x)
    h = HF.nchw_to_tokens(mod.net[2](HF.tokens_to_nchw(h, *hw)))
    return mod.net[6](HF.gelu(h))


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
    return f"{statistics.median(ts):8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " | ".join(l.strip() for l in out.splitlines() if "sclk" in l or "mclk" in l)[:400] or "not reported"
    except Exception as e:  # the tool is not installed / not permitted: say so, do not guess
        return f"not read ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r17", "mixff_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mixff_bench needs the MI355X"
    dev = "cuda:0"
    lines = [f"mixff_bench: {torch.cuda.get_device_name(0)}; clocks before: {clocks()}",
             f"{args.windows} windows of {args.iters} calls per path, alternating; median (min, max) per call"]
    for b, h, w, d, lat in SHAPES:
        torch.manual_seed(0)
        mod = M.MixFeedForward(d, lat, 0.0).to(dev)
        hw = (h, w)
        x = torch.randn(b, h * w, d, device=dev).to(torch.bfloat16)
        dy = torch.randn(b, h * w, d, device=dev).to(torch.bfloat16)
        with torch.no_grad():
            ya, yb = mod(x, hw=hw).float(), composed(mod, x, hw).float()
        lines.append(f"\nB {b}, tokens {h} x {w}, in_dim {d}, latent {lat}: outputs rel-L2 fused vs composed {((ya - yb).norm() / yb.norm()).item():.2e}")

        def fwd(f):
            with torch.no_grad():
                f(x)

        def fwd_bwd(f):
            xg = x.detach().requires_grad_()
            f(xg).backward(dy)

        fa, fb = (lambda t: mod(t, hw=hw)), (lambda t: composed(mod, t, hw))
        for name, run in (("forward", fwd), ("forward + backward", fwd_bwd)):
            ta, tb = ab(lambda: run(fa), lambda: run(fb), args.iters, args.windows)
            lines.append(f"  {name:18s} fused {fmt(ta)}   composed {fmt(tb)}   composed / fused {statistics.median(tb) / statistics.median(ta):.2f}")
        # the two convolution launches alone
        m = b * h * w
        rows, dyr = torch.randn(m, lat, device=dev).to(torch.bfloat16), torch.randn(m, lat, device=dev).to(torch.bfloat16)
        conv = mod.net[2].net
        wf, bf = conv.weight.detach(), conv.bias.detach()
        dw, db = torch.empty_like(wf), torch.empty_like(bf)
        tf, tb = ab(lambda: ops.dwconv3x3_rows_fwd(rows, wf, bf, b, h, w, 1),
                    lambda: ops.dwconv3x3_rows_bwd(dyr, rows, wf, bf, b, h, w, 1, dw=dw, db=db), args.iters, args.windows)
        for name, ts, passes in (("conv + GELU fwd", tf, 2), ("conv + GELU bwd", tb, 3)):
            nbytes = passes * m * lat * 2
            lines.append(f"  {name:18s} {fmt(ts)}   minimum traffic {nbytes / 1e6:.1f} MB -> {nbytes / statistics.median(ts) / 1e6:.0f} GB/s")
    lines.append(f"\nclocks after: {clocks()}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
