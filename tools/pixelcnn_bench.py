"""Two A/Bs of the PixelCNN prior on the MI355X, each alternating in one process.

1. Sampling: `PixelCNN.sample` (the preparation and ONE cfhip_pixelcnn_sample launch over all pixels,
csrc/pixelcnn.hip) against the reference's loop (pixel_cnn.py:160-164: one full forward of this same module per pixel, softmax and
torch.multinomial of that pixel's logits), alternating in one process.

    python tools/pixelcnn_bench.py [--out profiles/r12/pixelcnn_ab.txt] [--rounds 5]

Module: the reference's defaults (latent_channels = 128, 6 layers, BatchNorm, channel padding 16) with num_codes = 512, eval mode.
Workloads: 32^2 x 16 samples and 16^2 x 64 samples.  Every figure is the median over `rounds` alternating rounds of one whole
sampling call between device events, with the min .. max of the rounds as its spread; the shader clock and socket power averaged over
each variant's timed rounds come from tools/gpu_telemetry.py.  Also printed: the walk alone (the one launch, without the
preparation), per pixel, and the bytes of filter packs a workgroup streams per pixel.

2. Training: forward + backward (dX and dW) of ONE mask-"B" layer, 128 -> 128 channels, no bias, at 32^2 x 64 and 16^2 x 16: the
live-tap route (`pixelcnn.MaskedConv2dFn`, csrc/conv_masked.hip) against `Conv2dFn` on the zeroed weight (`functional.MASKED_CONV =
False`: the im2row route with all 49 taps).  `--inner` back-to-back calls per timing.  The selection rule: the live-tap route ships
only if it is faster at BOTH shapes; the verdict is the last line of the file.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd import functional as HF  # noqa: E402
from tools.gpu_telemetry import GpuTelemetry  # noqa: E402

DEV = "cuda"
WORKLOADS = [(16, 32), (64, 16)]  # (samples, img_size)
NUM_CODES = 512


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, rounds, tel):
    """{name: dict(ms=(median, min, max), sclk_mhz, power_w)} of callables run in alternating rounds (one warm-up call each first)"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    spans = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            ms[name].append(timed(fn))
            spans[name].append((t0, time.perf_counter()))
    out = {}
    for name, v in ms.items():
        sums = [tel.summary(t0, t1) for t0, t1 in spans[name]] if tel.available else []
        avg = lambda key: (lambda xs: round(sum(xs) / len(xs), 1) if xs else None)([s[key] for s in sums if s.get(key) is not None])  # noqa: E731
        out[name] = dict(ms=(statistics.median(v), min(v), max(v)), sclk_mhz=avg("sclk_mhz_avg"), power_w=avg("power_w_avg"))
    return out


def fmt(name, r):
    m, lo, hi = r["ms"]
    return f"{name} {m:9.2f} ms ({lo:.2f} .. {hi:.2f}) sclk {r['sclk_mhz']} MHz {r['power_w']} W"


@torch.no_grad()
def reference_loop(model, num_samples, img_size):
    """pixel_cnn.py:150-165 on this package's module: img_size^2 full forwards"""
    sampled = torch.zeros((num_samples, 1, img_size, img_size), dtype=torch.long, device=DEV)
    for i in range(img_size):
        for j in range(img_size):
            out = model(sampled, None)
            probabilities = torch.softmax(out[:, :, i, j].float(), dim=1)
            sampled[:, :, i, j] = torch.multinomial(probabilities, 1)
    return sampled


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "pixelcnn_ab.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixelcnn_bench.py measures on the MI355X: no HIP device here")
    tel = GpuTelemetry(0).start()
    torch.manual_seed(0)
    model = C.PixelCNN(NUM_CODES, 1).to(DEV).eval()
    c, nl = model.latent_channels, model.num_layers
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; PixelCNN(num_codes={NUM_CODES}, latent_channels={c}, "
             f"num_layers={nl}), eval; one whole sampling call per timing; rounds {args.rounds}; ms: median (min .. max over the alternating "
             f"rounds); telemetry: {tel.source.name if tel.available else 'unavailable (' + str(tel.error) + ')'}"]
    results: dict = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for b, size in WORKLOADS:
        key = f"B{b}_S{size}"
        r = alternate({"hip_sample": lambda: model.sample(b, img_size=size, seed=1),
                       "forward_per_pixel": lambda: reference_loop(model, b, size)}, args.rounds, tel)
        ratio = r["forward_per_pixel"]["ms"][0] / r["hip_sample"]["ms"][0]
        lines.append(f"{size}^2 x {b}   " + "   ".join(fmt(n, v) for n, v in r.items()) + f"   loop / sample {ratio:.1f}x")
        plan = model.sampler_plan(None, b)
        state = model.sampler_state(b, size)
        k = alternate({"walk": lambda: model.sample_pixels(plan, state, 0, size * size, seed=1)}, args.rounds, tel)
        per_pixel = k["walk"]["ms"][0] / (size * size) * 1e3
        stream = plan.packs.numel() * 2 + plan.head_pack.numel() * 2
        lines.append(f"   the walk alone: {fmt('pixelcnn_sample', k['walk'])}   = {per_pixel:.1f} us per pixel; {(b + 15) // 16} workgroup(s), "
                     f"each streams {stream} B of packs per pixel")
        results[key] = dict(r, walk=k["walk"], us_per_pixel=per_pixel, pack_bytes_per_pixel=stream, workgroups=(b + 15) // 16)
        print("\n".join(lines[-2:]), flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(results) + "\n")
    # ---- 2. one mask-"B" layer, forward + backward ----
    wins = []
    for b, size in ((64, 32), (16, 16)):
        torch.manual_seed(1)
        conv = C.MaskedConv2d("B", c, c, kernel_size=7, padding=3, bias=False).to(DEV)
        x = torch.randn(b, c, size, size, device=DEV).to(torch.bfloat16).requires_grad_(True)
        dy = torch.randn(b, c, size, size, device=DEV).to(torch.bfloat16)

        def step(masked):
            def go():
                HF.MASKED_CONV = masked
                try:
                    for _ in range(args.inner):
                        conv.weight.grad = None
                        x.grad = None
                        conv(x).backward(dy)
                        HF.SideStream.join()
                finally:
                    HF.MASKED_CONV = True
            return go

        r = alternate({"live_taps": step(True), "conv2d_zeroed_weight": step(False)}, args.rounds, tel)
        for v in r.values():
            v["ms"] = tuple(t / args.inner for t in v["ms"])
        ratio = r["conv2d_zeroed_weight"]["ms"][0] / r["live_taps"]["ms"][0]
        wins.append(ratio > 1.0)
        lines.append(f"mask B layer {c} -> {c}, fwd + bwd, {size}^2 x {b}   " + "   ".join(fmt(n, v) for n, v in r.items())
                     + f"   conv2d / live taps {ratio:.2f}x")
        results[f"train_B{b}_S{size}"] = r
        print(lines[-1], flush=True)
    lines.append("selection rule (the live-tap route ships only if faster at both shapes): " + ("SHIPS" if all(wins) else "DOES NOT SHIP"))
    print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n" + json.dumps(results) + "\n")
    tel.stop()
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
