"""A/B of the ControlNet hint block's convolutions on the MI355X: the direct kernel (functional.DirectConv3x3Fn) against the route
Conv2dFn gives the same layer, alternating in one process.

    python tools/controlnet_bench.py [--out profiles/r08/controlnet_direct_ab.txt] [--rounds 7] [--inner 200] [--no-step]

  1. the five narrow hint layers at 512^2 x 8 (each at the resolution it has inside the block), forward and input gradient, device
     events: DirectConv3x3Fn | Conv2dFn forced onto IM2ROW | (32 -> 32 only) Conv2dFn on the route it takes today, IMPLICIT.  The
     weights are frozen for this part, so a backward is the input gradient alone (the weight gradient is shared code).
  2. the whole hint block, forward + backward with weight gradients, `functional.DIRECT_HINT_CONV` on and off.
  3. one ControlNetTrainStep at the zoo configuration (start_channels 320, multipliers (1, 2, 4, 4) as in bench.py's UNet workload — the
     reference default (1, 2, 4, 8) puts 2560 channels into the middle block's LayerNorm, past the kernel's 2048 —, 64^2 x 8 latent,
     512^2 hint, 77 x 768 context), both ways.
Every figure is the median over `rounds` alternating rounds of back-to-back calls (per call), with the min .. max of the rounds as
its spread: `inner` calls per round for a layer (200: a window of 10 ms and more), inner / 20 for the hint block, 2 train steps.
The per-layer rows of 1 are PER-CALL times of the autograd function — filter pack, channel padding and layout transposes
included, with their launches —, not kernel times; the "kernel alone" row times cfhip_conv3x3_direct_bf16 by itself on prepared
operands and gives the bytes it must move (input + output activation, bf16) over that time and over the 8.0 TB/s HBM peak (the
kernel is bandwidth-bound: 2 x 9 x Cp x N FLOP per output pixel against 2 (Cp / s^2 + N) bytes).  Needs the GPU: there is no CPU
path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd import functional as HF  # noqa: E402
from cflearn_amd.diffusion import ControlNetTrainStep, NoiseSchedule  # noqa: E402
from cflearn_amd.modules import UNetDiffuser  # noqa: E402

DEV = "cuda"
LAYERS = [(3, 16, 1, 512), (16, 16, 1, 512), (16, 32, 2, 512), (32, 32, 1, 256), (32, 96, 2, 256)]  # (Cin, Cout, stride, input side)
BATCH = 8
ZOO = dict(num_heads=8, use_spatial_transformer=True, context_dim=768, channel_multipliers=(1, 2, 4, 4))


def timed(fn, inner):
    """ms per call of `inner` back-to-back calls, between device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(variants, rounds, inner):
    """{name: (median, min, max)} of callables run in alternating rounds (one warm-up round first)"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(timed(fn, inner))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def fmt(r):
    return "  ".join(f"{name} {m:8.3f} ms ({lo:.3f} .. {hi:.3f})" for name, (m, lo, hi) in r.items())


def layer_ab(cin, cout, stride, side, rounds, inner, lines, results):
    gen = torch.Generator().manual_seed(cin * 100 + cout)
    w = (torch.randn((cout, cin, 3, 3), generator=gen) * (9 * cin) ** -0.5).to(DEV)
    bias = torch.randn((cout,), generator=gen).to(DEV)
    if cin == 3:  # the hint itself: f32 NCHW, no gradient
        x = torch.rand((BATCH, cin, side, side), generator=gen).to(DEV)
    else:  # an activation of the block: bf16 NHWC
        x = HF.to_nhwc(torch.randn((BATCH, cin, side, side), generator=gen).to(DEV)).detach().requires_grad_(True)
    so = (side - 1) // stride + 1
    dy = HF.to_nhwc(torch.randn((BATCH, cout, so, so), generator=gen).to(DEV)).detach()

    def run(direct, implicit):
        def fwd():
            HF.IMPLICIT_CONV = implicit
            return HF.direct_conv3x3(x, w, bias, stride) if direct else HF.Conv2dFn.apply(x, w, bias, stride, 1, 1)
        return fwd

    names = {"direct": run(True, True), "im2row": run(False, False)}
    if HF.conv_route(cin, cout, 3, 3, stride, 1, 1, side, side)[0] == HF.IMPLICIT:
        names["implicit"] = run(False, True)
    keep = HF.IMPLICIT_CONV
    prev = HF.NHWC[0]
    HF.NHWC[0] = True
    try:
        f = alternate(names, rounds, inner)
        lines.append(f"{cin:3d} -> {cout:3d} s{stride} {side}^2 x {BATCH}  forward         {fmt(f)}")
        results[f"{cin}x{cout}s{stride}"] = {"forward": f}
        x4 = HF.nhwc_rows(HF.pad_hint_nhwc(x.detach())).view(BATCH, side, side, -1)
        wp = HF.ops.conv3x3_direct_pack(w, 0)
        k = alternate({"kernel": lambda: HF.ops.conv3x3_direct(x4, wp, bias, side, side, stride, 0)}, rounds, inner)["kernel"]
        nbytes = 2 * BATCH * (side * side * x4.shape[3] + so * so * cout)
        lines.append(f"{cin:3d} -> {cout:3d} s{stride} {side}^2 x {BATCH}  kernel alone    {k[0]:8.3f} ms ({k[1]:.3f} .. {k[2]:.3f})  {nbytes / 1e6:.1f} MB  "
                     f"{nbytes / k[0] / 1e9:.2f} TB/s = {nbytes / k[0] / 1e9 / 8.0:.2f} of the HBM peak")
        results[f"{cin}x{cout}s{stride}"].update(kernel=k, kernel_bytes=nbytes)
        if cin != 3:
            def bwd_of(fwd):
                def go():
                    x.grad = None
                    fwd().backward(dy)
                return go
            fb = alternate({k: bwd_of(v) for k, v in names.items()}, rounds, inner)
            b = {k: tuple(t - f[k][i] for i, t in enumerate(fb[k])) for k in fb}  # (forward + backward) - forward, per statistic
            lines.append(f"{cin:3d} -> {cout:3d} s{stride} {side}^2 x {BATCH}  forward+dX      {fmt(fb)}")
            lines.append(f"{cin:3d} -> {cout:3d} s{stride} {side}^2 x {BATCH}  dX (difference) " + "  ".join(f"{k} {v[0]:8.3f} ms" for k, v in b.items()))
            results[f"{cin}x{cout}s{stride}"].update(forward_dx=fb)
    finally:
        HF.IMPLICIT_CONV = keep
        HF.NHWC[0] = prev


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "controlnet_direct_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("controlnet_bench.py measures on the MI355X: no HIP device here")
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; rounds {args.rounds} x inner {args.inner}; "
             "ms per call: median (min .. max over the rounds); layer rows: the whole autograd call (pack, padding, transposes), not kernel time"]
    results: dict = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    shown = 0

    def flush() -> None:  # (after every section: a later failure keeps what was measured)
        nonlocal shown
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(results) + "\n")

    for cin, cout, stride, side in LAYERS:
        layer_ab(cin, cout, stride, side, args.rounds, args.inner, lines, results)
        flush()
    torch.manual_seed(0)
    with torch.device(DEV):
        cn = C.ControlNet(4, 3, **ZOO)
    hint = torch.rand((BATCH, 3, 512, 512), device=DEV)
    gh = torch.randn((BATCH, 320, 64, 64), device=DEV).bfloat16()

    def block(direct):
        def go():
            HF.DIRECT_HINT_CONV = direct
            prev = HF.NHWC[0]
            HF.NHWC[0] = True
            try:
                cn._guided_hint(hint).backward(HF.to_nhwc(gh))
                HF.SideStream.join()
            finally:
                HF.NHWC[0] = prev
        return go

    r = alternate({"direct": block(True), "conv2dfn": block(False)}, args.rounds, max(1, args.inner // 20))
    lines.append(f"hint block forward + backward, 512^2 x {BATCH}            {fmt(r)}")
    results["hint_block"] = r
    flush()
    if not args.no_step:
        with torch.device(DEV):
            unet = UNetDiffuser(4, 4, **ZOO)
        ts = ControlNetTrainStep(unet, cn, NoiseSchedule(device=DEV), lr=1e-5)
        x = torch.randn((BATCH, 4, 64, 64), device=DEV)
        ctx = torch.randn((BATCH, 77, 768), device=DEV)

        def step(direct):
            def go():
                HF.DIRECT_HINT_CONV = direct
                ts.step(x, hint, ctx)
            return go

        r = alternate({"direct": step(True), "conv2dfn": step(False)}, args.rounds, 2)
        lines.append(f"ControlNetTrainStep, zoo configuration, 64^2 x {BATCH} latent {fmt(r)}")
        results["train_step"] = r
        flush()
    HF.DIRECT_HINT_CONV = True
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
