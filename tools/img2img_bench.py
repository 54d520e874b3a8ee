"""What a reference costs a sampler step: DDIM on the latent zoo UNet (diffusion/ddpm widths: start 320, multipliers 1/2/4/4, 4 latent
channels in and out, a 768-wide context) at 64 x 64 latents, batch 8, as a recorded graph, with and without `ref` / `ref_mask`
(a half-plane mask with a fractional edge, a fresh Philox draw per merge), alternating in one process after a warm-up run of
each.  Device events around each whole run; ms per step = run / steps.

    python tools/img2img_bench.py [--steps 50] [--repeats 5] [--guidance off|on] [--eager]

`--launch-only N`: the step launch alone, `cfhip_diffusion_sample_step` against `cfhip_diffusion_sample_step_ref` on the same
state, N launches each per block, blocks alternating: microseconds per launch (the merge's own cost, without the UNet).

For launches per run, run one form alone under `rocprofv3 --kernel-trace --stats` with --forms plain|ref --eager --repeats 1
--no-warmup and count the dispatches: the two forms differ by the one stand-alone merge in front of the first step."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd import ops  # noqa: E402
from cflearn_amd.diffusion import NoiseSchedule, make_sampler, sampler_side_table, sampler_table  # noqa: E402


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def launch_only(args, dev) -> None:
    b, shape = args.batch, (args.batch, 4, args.img, args.img)
    g = torch.Generator().manual_seed(2)
    sched = NoiseSchedule(device=dev)
    table = sampler_table("ddim", sched, args.steps).to(dev)
    side = sampler_side_table("ddim", sched, args.steps).to(dev)
    x0 = torch.randn(shape, generator=g).to(dev)
    ref = torch.randn(shape, generator=g).to(dev)
    col = torch.zeros(args.img)
    col[:args.img // 2 - 1], col[args.img // 2 - 1] = 1.0, 0.5
    mask = col.repeat(args.img, 1).view(1, 1, args.img, args.img).contiguous().to(dev)
    out = torch.randn(shape, generator=g).to(dev).bfloat16()
    xin = torch.empty(shape, dtype=torch.bfloat16, device=dev)
    k = torch.zeros((1,), dtype=torch.int32, device=dev)
    kw = dict(kind="ddim", parameterization="eps", seed=1, offset=x0.numel() // 4)
    x = x0.clone()
    forms = {
        "plain": lambda: ops.diffusion_sample_step(x, xin, out, table, k, **kw),
        "ref": lambda: ops.diffusion_sample_step_ref(x, xin, out, table, k, ref=ref, mask=mask, side=side, **kw),
    }
    n = args.launch_only
    for f in forms.values():
        for _ in range(20):
            f()
    times = {f: [] for f in forms}
    for _ in range(args.repeats):
        for name, f in forms.items():
            x.copy_(x0)

            def block(f=f):
                for _ in range(n):
                    f()

            times[name].append(timed(block) * 1000.0 / n)
    for name, t in times.items():
        print(json.dumps(dict(what="step launch alone", form=name, batch=b, img=args.img, elements=x0.numel(), launches_per_block=n,
                              us_per_launch_median=round(statistics.median(t), 3), us_per_launch_min=round(min(t), 3),
                              us_per_launch_max=round(max(t), 3), repeats=len(t))), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forms", default="plain,ref")
    ap.add_argument("--guidance", default="off", choices=["on", "off"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--img", type=int, default=64)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--launch-only", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.launch_only:
        launch_only(args, dev)
        return
    torch.manual_seed(0)
    cfg = dict(in_channels=4, out_channels=4, start_channels=320, num_heads=8, use_spatial_transformer=True,
               num_transformer_layers=1, num_res_blocks=2, attention_downsample_rates=(1, 2, 4),
               channel_multipliers=(1, 2, 4, 4), context_dim=768)
    m = C.build_module("unet_diffuser", config=cfg).to(dev)
    g = torch.Generator().manual_seed(1)
    b = args.batch
    shape = (b, 4, args.img, args.img)
    z, ref = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    col = torch.zeros(args.img)
    col[:args.img // 2 - 1], col[args.img // 2 - 1] = 1.0, 0.5
    mask = col.repeat(args.img, 1).view(1, 1, args.img, args.img).contiguous().to(dev)
    cond = torch.randn(b, 77, 768, generator=g).to(dev)
    uncond = torch.randn(1, 77, 768, generator=g)
    scale = 7.5 if args.guidance == "on" else 1.0
    s = make_sampler("ddim", m, NoiseSchedule(device=dev), unconditional_cond=uncond, unconditional_guidance_scale=scale)
    kw = dict(cond=cond, num_steps=args.steps, seed=3, use_graph=not args.eager)
    runs = {
        "plain": lambda: s.sample_with_reference(z, **kw),
        "ref": lambda: s.sample_with_reference(z, ref=ref, ref_mask=mask, **kw),
    }
    forms = [f for f in args.forms.split(",") if f in runs]
    if not args.no_warmup:
        for f in forms:
            runs[f]()
        torch.cuda.synchronize()
    times = {f: [] for f in forms}
    for _ in range(args.repeats):
        for f in forms:
            times[f].append(timed(runs[f]) / args.steps)
    for f in forms:
        t = times[f]
        print(json.dumps(dict(what="ddim sampler step", form=f, graph=not args.eager, guidance=args.guidance, batch=b, img=args.img,
                              steps=args.steps, ms_per_step_median=round(statistics.median(t), 3), ms_per_step_min=round(min(t), 3),
                              ms_per_step_max=round(max(t), 3), repeats=len(t))), flush=True)


if __name__ == "__main__":
    main()
