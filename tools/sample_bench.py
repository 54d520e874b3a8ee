"""Sampling time of the zoo DDPM UNet (diffusion/ddpm: start 320, multipliers 1/2/4/4, with a 768-wide context so that
guidance has a condition) at 64^2 x 8, DDIM 50 steps, without guidance and with guidance at scale 7.5, in three forms within
one process:
  (a) the path a user has today: the reference sampler's arithmetic (samplers/ddim.py:195-239, schema.py:197-263) as
      plain torch ops around the eager HIP UNet;
  (b) the eager HIP sampler (diffusion.make_sampler, one fused step kernel + one advance launch per step);
  (c) the same as a recorded graph (use_graph=True).
Device events around each whole run after a warm-up run of every form; the forms alternate; ms per step = run / steps.

    python tools/sample_bench.py [--steps 50] [--repeats 3] [--forms abc] [--guidance both|on|off]

`--kind k_euler_a | k_heun | k_dpmpp_2m` times a sigma-space sampler instead (default 25 steps, as the reference's; form (a) is then
samplers/k_samplers.py's arithmetic, its `.item()` reads included, around the same HIP UNet with float timesteps); a run of N
steps makes N - 1 steps that evaluate the model, and ms per step = run / (N - 1).

For launches per step, run one form alone under `rocprofv3 --kernel-trace --stats` with --repeats 1 --no-warmup."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cflearn_amd as C  # noqa: E402
from cflearn_amd.diffusion import NoiseSchedule, ddim_tables, get_ancestral_step, k_sigma_tables, k_sigma_to_t, make_sampler  # noqa: E402


def torch_ddim(unet, sched, z, cond, uncond, scale, steps):
    """(a): DDIMSampler.sample_step's arithmetic as the reference runs it, one ATen op at a time, around the HIP UNet"""
    tb = ddim_tables(sched, steps)
    dev = z.device
    a, ap, sg, s1m = (tb[k].to(dev) for k in ("alphas", "alphas_prev", "sigmas", "sqrt_one_minus_alphas"))
    b = z.shape[0]
    x = z
    guided = uncond is not None and scale != 1.0
    uc = uncond.repeat_interleave(b, dim=0) if guided else None
    with torch.no_grad():
        for step in range(steps):
            i = steps - step - 1
            ts = torch.full((b,), tb["timesteps"][i], device=dev, dtype=torch.long)
            ext = lambda v: torch.full((b, 1, 1, 1), 0.0, device=dev).copy_(v[i].expand(b, 1, 1, 1))  # noqa: E731
            at, a_prev, sig, sq = ext(a), ext(ap), ext(sg), ext(s1m)
            if guided:
                out = unet(torch.cat([x, x]), timesteps=torch.cat([ts, ts]), context=torch.cat([cond, uc])).float()
                e_c, e_u = out.chunk(2)
                eps = e_u + scale * (e_c - e_u)
            else:
                eps = unet(x, timesteps=ts, context=cond).float()
            x0 = (x - sq * eps) / at.sqrt()
            direction = (1.0 - a_prev - sig ** 2).sqrt() * eps
            noise = sig * torch.randn_like(x) * 1.0
            x = a_prev.sqrt() * x0 + direction + noise
    return torch.clip(x, -1.0, 1.0)


def torch_k(kind, unet, sched, z, cond, uncond, scale, steps):
    """(a) for the sigma-space samplers: IKSampler.sample_step's get_denoised (eps) and the three `sample_step_core`s
    (samplers/k_samplers.py:127-203,367-477) as the reference runs them, one ATen op at a time, around the HIP UNet"""
    dev = z.device
    tb = k_sigma_tables(sched, steps)
    sigmas, log_base = tb["sigmas"].to(dev), tb["log_sigmas_base"].to(dev)
    b = z.shape[0]
    guided = uncond is not None and scale != 1.0
    uc = uncond.repeat_interleave(b, dim=0) if guided else None
    t_fn = lambda sg: sg.log().neg()  # noqa: E731

    def get_denoised(img, sigma):
        sigma = sigma * s_in
        ts = k_sigma_to_t(sigma, log_base, False)
        c_in = (1.0 / (sigma ** 2 + 1.0) ** 0.5)[:, None, None, None]
        c_out = sigma[:, None, None, None]
        inp = img * c_in
        if guided:
            out = unet(torch.cat([inp, inp]), timesteps=torch.cat([ts, ts]), context=torch.cat([cond, uc])).float()
            e_c, e_u = out.chunk(2)
            eps = e_u + scale * (e_c - e_u)
        else:
            eps = unet(inp, timesteps=ts, context=cond).float()
        return img - eps * c_out

    with torch.no_grad():
        image = z * sigmas[0]
        s_in = image.new_ones([b])
        old_denoised = None
        for step in range(steps - 1):
            sigma, next_sigma = sigmas[step], sigmas[step + 1]
            if kind == "k_euler_a":
                denoised = get_denoised(image, sigma)
                sigma_down, sigma_up = get_ancestral_step(sigma.item(), next_sigma.item(), eta=1.0)
                d = (image - denoised) / sigma
                image = image + d * (sigma_down - sigma)
                if next_sigma.item() > 0:
                    image = image + torch.randn_like(image) * 1.0 * sigma_up
            elif kind == "k_heun":
                sigma.item()
                eps = torch.randn_like(image) * 1.0  # noqa: F841  (drawn and unused, as in the reference)
                sigma_hat = sigma * 1.0
                denoised = get_denoised(image, sigma_hat)
                d = (image - denoised) / sigma_hat
                dt = next_sigma - sigma_hat
                if next_sigma.item() == 0:
                    image = image + d * dt
                else:
                    x_2 = image + d * dt
                    d_2 = (x_2 - get_denoised(x_2, next_sigma)) / next_sigma
                    image = image + ((d + d_2) / 2) * dt
            else:
                denoised = get_denoised(image, sigma)
                t, t_next = t_fn(sigma), t_fn(next_sigma)
                h = t_next - t
                if old_denoised is None or next_sigma.item() == 0:
                    image = (next_sigma / sigma) * image - (-h).expm1() * denoised
                else:
                    r = (t - t_fn(sigmas[step - 1])) / h
                    dd = (1 + 1 / (2 * r)) * denoised - (1 / (2 * r)) * old_denoised
                    image = (next_sigma / sigma) * image - (-h).expm1() * dd
                old_denoised = denoised
    return torch.clip(image, -1.0, 1.0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="ddim", choices=["ddim", "k_euler_a", "k_heun", "k_dpmpp_2m"])
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forms", default="abc")
    ap.add_argument("--guidance", default="both", choices=["both", "on", "off"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--img", type=int, default=64)
    ap.add_argument("--no-warmup", action="store_true")
    args = ap.parse_args()
    ddim = args.kind == "ddim"
    if args.steps is None:
        args.steps = 50 if ddim else 25
    per_run = args.steps if ddim else args.steps - 1  # steps that evaluate the model
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = dict(in_channels=3, out_channels=3, start_channels=320, num_heads=8, use_spatial_transformer=True,
               num_transformer_layers=1, num_res_blocks=2, attention_downsample_rates=(1, 2, 4),
               channel_multipliers=(1, 2, 4, 4), context_dim=768)
    m = C.build_module("unet_diffuser", config=cfg).to(dev)
    nparam = sum(p.numel() for p in m.parameters())
    g = torch.Generator().manual_seed(1)
    b = args.batch
    z = torch.randn(b, 3, args.img, args.img, generator=g).to(dev)
    cond = torch.randn(b, 77, 768, generator=g).to(dev)
    uncond = torch.randn(1, 77, 768, generator=g)
    sched = NoiseSchedule(device=dev)
    cases = {"off": 1.0, "on": 7.5}
    if args.guidance != "both":
        cases = {args.guidance: cases[args.guidance]}
    for name, scale in cases.items():
        s = make_sampler(args.kind, m, sched, unconditional_cond=uncond, unconditional_guidance_scale=scale)
        runs = {
            "a": (lambda: torch_ddim(m, sched, z, cond, uncond.to(dev), scale, args.steps)) if ddim else
                 (lambda: torch_k(args.kind, m, sched, z, cond, uncond.to(dev), scale, args.steps)),
            "b": lambda: s.sample(z, cond=cond, num_steps=args.steps),
            "c": lambda: s.sample(z, cond=cond, num_steps=args.steps, use_graph=True),
        }
        forms = [f for f in args.forms if f in runs]
        if not args.no_warmup:
            for f in forms:
                runs[f]()
            torch.cuda.synchronize()
        times = {f: [] for f in forms}
        for _ in range(args.repeats):
            for f in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                runs[f]()
                e1.record()
                torch.cuda.synchronize()
                times[f].append(e0.elapsed_time(e1) / per_run)
        for f in forms:
            t = times[f]
            print(json.dumps(dict(kind=args.kind, form=f, guidance=name, scale=scale, batch=b, img=args.img, steps=args.steps, params=nparam,
                                  ms_per_step_median=round(statistics.median(t), 3), ms_per_step_min=round(min(t), 3),
                                  ms_per_step_max=round(max(t), 3), repeats=len(t))), flush=True)


if __name__ == "__main__":
    main()
