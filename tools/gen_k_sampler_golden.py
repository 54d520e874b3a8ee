"""Generate tests/golden/k_samplers.pt: the reference's own sigma-space samplers (samplers/k_samplers.py: k_euler_a, k_heun,
k_dpmpp_2m) run on the CPU.

    python tools/gen_k_sampler_golden.py

Needs the reference tree (oracle/refharness finds it); writes data only.  Contents:
  * tables: `IKSampler._reset_buffers` (k_samplers.py:248-269) for sigmas_scheduler {None, karras} x quantize {off, on} x
    {8, 25} steps: `sigmas` (the appended zero included) and the timestep `_sigma_to_t` makes of each sigma the way
    `get_denoised` asks for it (`sigma * s_in`, a [B] tensor); `sigmas_base` and `log_sigmas_base` once;
  * steps: {k_euler_a, k_heun, k_dpmpp_2m} x {eps / default sigmas / float timesteps, v / karras / quantised} x guidance
    {off, 7.5} on a seeded [2, 3, 16, 16] state and 8 steps (7 of them evaluate the model, k_heun twice), the reference's
    `ISampler.sample` over a stand-in model whose `denoise` returns seeded bf16-representable outputs; every model output, the
    timesteps every `denoise` call received, every `torch.randn_like` draw of k_euler_a and the scalars of every evaluation are
    recorded (`table`, columns `columns`: formed here with the reference's own buffers, methods and expressions);
  * e2e: per kind the reference `UNetDiffuser` with the weights of tests/golden/unet_small.pt (not stored again): 12 steps,
    guidance 3.0 with an unconditional context, eps / linear, default sigmas, float timesteps, in fp32 and under CPU bf16
    autocast (the reference's own mixed-precision distance), with recorded noise for k_euler_a.
Single-threaded and seeded: a second run writes the same bytes.

As in tools/gen_sampler_golden.py the model outputs and the noise are drawn on coarse grids and stored as int8 codes (outputs
k / 64, |k| <= 96; draws a sum of four seeded integers in [-31, 31] over 32), and the intermediate images of the step records are
stored as the SHA-256 of their f32 bytes: the tests rebuild the chain from `step_z` with the kernel's operation order in numpy
f32 and check every image against it."""
import hashlib
import importlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from refharness import import_cflearn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "k_samplers.pt")
OUTPUT_SCALE, NOISE_SCALE = 1.0 / 64, 1.0 / 32
COLUMNS = ("t", "sigma", "c_out", "c_skip", "c_in_next", "dt", "sigma_up", "sigma_ratio", "expm1_neg_h", "r_plus", "r_minus", "flag")


def codes(ts, scale):
    """int8 codes of values on the grid `scale` (exact: checked)"""
    t = torch.stack(ts) if isinstance(ts, (list, tuple)) else ts
    q = torch.round(t / scale)
    assert q.abs().max() <= 127 and torch.equal(q * scale, t)
    return q.to(torch.int8)


def main() -> None:
    torch.set_num_threads(1)
    import_cflearn()
    ddpm_mod = sys.modules["cflearn.modules.multimodal.diffusion.ddpm"]
    k_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.samplers.k_samplers")
    unet_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.unet")
    DDPM = ddpm_mod.DDPM
    classes = dict(k_euler_a=k_mod.KEulerAncestralSampler, k_heun=k_mod.KHeunSampler, k_dpmpp_2m=k_mod.KDPMpp2MSampler)

    class StandIn(torch.nn.Module):
        """exactly what the samplers read off a DDPM: the schedule buffers, parameterization, condition_model / get_cond
        (identity), denoise"""

        def __init__(self, parameterization: str, schedule: str = "linear"):
            super().__init__()
            self.parameterization, self.v_posterior = parameterization, 0.0
            self.anchor = torch.nn.Parameter(torch.zeros(1))
            DDPM._register_noise_schedule(self, 1000, None, schedule, 8.5e-4, 1.2e-2, 8.0e-3)
            self.condition_model = object()
            self.get_cond = lambda c: c

    out: dict = {"tables": [], "steps": [], "e2e": {}, "columns": COLUMNS}
    # ---- tables
    m = StandIn("eps")
    for sched in (None, "karras"):
        for quantize in (False, True):
            for steps in (8, 25):
                s = k_mod.KEulerAncestralSampler(m, default_quantize=quantize, sigmas_scheduler=sched)
                s._reset_buffers(steps, quantize, None, 1.0, sched)
                ts = torch.stack([s._sigma_to_t(s.sigmas[i] * torch.ones(2), quantize)[0] for i in range(steps)])
                out["tables"].append(dict(sigmas_scheduler=sched, quantize=quantize, steps=steps, sigmas=s.sigmas.clone(),
                                          timesteps=ts.clone()))
    out["sigmas_base"], out["log_sigmas_base"] = s.sigmas_base.clone(), s.log_sigmas_base.clone()

    real_randn_like = torch.randn_like
    noise_gen = torch.Generator().manual_seed(280)

    def near_normal(shape):
        q = sum(torch.randint(-31, 32, shape, generator=noise_gen) for _ in range(4))
        return q.float() * NOISE_SCALE

    def run(sampler, z, cond, steps, draws_in=None):
        """sampler.sample with every randn_like draw (a recorded near-normal one) and every step's image recorded (or the
        draws replayed)"""
        draws, images = [], [z.clone()]
        it = iter(draws_in) if draws_in is not None else None

        def randn_like(t, *a, **k):
            v = next(it).to(t.dtype) if it is not None else near_normal(t.shape).to(t.dtype)
            draws.append(v.clone())
            return v

        inner = sampler.sample_step

        def step(image, c, step_, total, *a, **k):
            r = inner(image, c, step_, total, *a, **k)
            images.append(r.detach().clone())
            return r

        sampler.sample_step = step
        torch.randn_like = randn_like
        try:
            y = sampler.sample(z, cond=cond, num_steps=steps, verbose=False)
        finally:
            torch.randn_like = real_randn_like
        return y.detach().clone(), draws, images

    def scalars(kind, par, s, steps, quantize):
        """one row per model evaluation, from the reference's buffers (`s.sigmas`), methods (`_sigma_to_t`, `t_fn`),
        `get_ancestral_step` and the expressions of k_samplers.py:152-183,384-397,419-440,464-477"""
        s_in = torch.ones(2)
        zero, one = torch.tensor(0.0), torch.tensor(1.0)

        def head(i, nxt):
            sigma = s.sigmas[i] * s_in
            ts = s._sigma_to_t(sigma, quantize)
            if par == "eps":
                c_out, c_skip = sigma, torch.ones(2)
            else:
                c_out = sigma * s.sigma_data / (sigma**2 + s.sigma_data**2) ** 0.5
                c_skip = s.sigma_data**2 / (sigma**2 + s.sigma_data**2)
            sigma_n = s.sigmas[nxt] * s_in
            c_in_n = 1.0 / (sigma_n**2 + s.sigma_data**2) ** 0.5
            return [ts[0].float(), sigma[0], c_out[0], c_skip[0], c_in_n[0]]

        rows = []
        for step in range(steps - 1):
            sigma, next_sigma = s.sigmas[step], s.sigmas[step + 1]
            if kind == "k_euler_a":
                sigma_down, sigma_up = k_mod.get_ancestral_step(sigma.item(), next_sigma.item(), eta=1.0)
                dt = sigma_down - sigma
                up = (torch.ones(1) * 1.0 * sigma_up)[0]  # `torch.randn_like(image) * s_noise * sigma_up`
                rows.append(head(step, step + 1) + [dt, up, zero, zero, zero, zero, one if next_sigma.item() > 0 else zero])
            elif kind == "k_heun":
                sigma_hat = sigma * (0.0 + 1)
                dt = next_sigma - sigma_hat
                rows.append(head(step, step + 1) + [dt, zero, zero, zero, zero, zero, zero])
                rows.append(head(step + 1, step + 1) + [dt, zero, zero, zero, zero, zero, one])
            else:
                t, t_next = map(s.t_fn, [sigma, next_sigma])
                h = t_next - t
                ratio, em1 = next_sigma / sigma, (-h).expm1()
                if step == 0:
                    rp, rm, flag = zero, zero, zero
                else:
                    h_last = t - s.t_fn(s.sigmas[step - 1])
                    r = h_last / h
                    rp, rm, flag = 1 + 1 / (2 * r), 1 / (2 * r), one
                rows.append(head(step, step + 1) + [zero, zero, ratio, em1, rp, rm, flag])
        return torch.stack([torch.stack([v.float().reshape(()) for v in r]) for r in rows])

    # ---- step records
    torch.manual_seed(250)
    z = torch.randn(2, 3, 16, 16)
    cond = torch.randn(2, 4, 8)
    uncond = torch.randn(1, 4, 8)
    ci = 0
    for kind in ("k_euler_a", "k_heun", "k_dpmpp_2m"):
        for par, sched, quantize in (("eps", None, False), ("v", "karras", True)):
            for scale in (None, 7.5):
                m = StandIn(par)
                gen = torch.Generator().manual_seed(260 + ci)
                ci += 1
                outputs, seen_ts = [], []

                def raw(image, ts, c, step, total, gen=gen, outputs=outputs, seen_ts=seen_ts):
                    o = torch.randint(-96, 97, image.shape, generator=gen).float() * OUTPUT_SCALE
                    outputs.append(o.clone())
                    seen_ts.append(ts.clone())
                    return o

                m.denoise = raw
                steps = 8
                s = classes[kind](m, default_quantize=quantize, sigmas_scheduler=sched, unconditional_cond=uncond,
                                  unconditional_guidance_scale=scale if scale is not None else 1.0)
                y, draws, images = run(s, z, cond if scale is not None else None, steps)
                assert torch.equal(y, images[-1]) and torch.equal(images[0], z) and torch.equal(images[-1], images[-2])
                s._reset_buffers(steps, quantize, None, 1.0, sched)  # (sample() leaves the buffers; rebuilt for the scalars)
                rows = scalars(kind, par, s, steps, quantize)
                assert rows.shape == (len(outputs), len(COLUMNS))
                ts_dtype = torch.int64 if quantize else torch.float32
                assert all(t.dtype == ts_dtype and bool((t == t[0]).all()) for t in seen_ts)
                tss = torch.stack([t[0] for t in seen_ts])
                assert torch.equal(tss.float(), rows[:, 0])
                rec = dict(kind=kind, parameterization=par, sigmas_scheduler=sched, quantize=quantize, scale=scale, steps=steps,
                           cond=cond.clone(), uncond=uncond.clone(), outputs_q=codes(outputs, OUTPUT_SCALE),
                           outputs_scale=OUTPUT_SCALE, table=rows, timesteps=tss, sigmas=s.sigmas.clone(),
                           image_sha256=[hashlib.sha256(im.contiguous().numpy().tobytes()).hexdigest() for im in images])
                if kind == "k_euler_a":  # (k_heun's draw is never used: not recorded)
                    assert len(draws) == steps - 1
                    rec.update(noises_q=codes(draws, NOISE_SCALE), noises_scale=NOISE_SCALE)
                out["steps"].append(rec)
    out["step_z"] = z.clone()
    # ---- end to end on the small UNet fixture
    u = torch.load(os.path.join(ROOT, "tests", "golden", "unet_small.pt"), map_location="cpu", weights_only=False)
    net = unet_mod.UNetDiffuser(**u["cfg"])
    net.load_state_dict(u["sd"])
    net.eval()
    torch.manual_seed(270)
    z = torch.randn(2, 3, 16, 16)
    cond = torch.randn(2, 5, 48)
    uncond = torch.randn(1, 5, 48)
    m = StandIn("eps")
    m.denoise = lambda image, ts, c, step, total: net(image, timesteps=ts, context=c)
    e2e = dict(z=z, cond=cond, uncond=uncond, steps=12, scale=3.0)
    with torch.no_grad():
        for kind in ("k_euler_a", "k_heun", "k_dpmpp_2m"):
            make = lambda: classes[kind](m, unconditional_cond=uncond, unconditional_guidance_scale=3.0)  # noqa: E731
            y, draws, _ = run(make(), z, cond, 12)
            e2e[f"{kind}_fp32"] = y
            if kind == "k_euler_a":
                e2e["k_euler_a_noise_q"], e2e["k_euler_a_noise_scale"] = codes(draws, NOISE_SCALE), NOISE_SCALE
            with torch.autocast("cpu", dtype=torch.bfloat16):
                e2e[f"{kind}_autocast"] = run(make(), z, cond, 12, draws_in=draws)[0].float()
            a, f = e2e[f"{kind}_autocast"], e2e[f"{kind}_fp32"]
            assert torch.isfinite(a).all() and torch.isfinite(f).all()
            d = (a - f).flatten(1).norm(dim=1) / f.flatten(1).norm(dim=1)
            print(f"{kind}: bf16-autocast vs fp32 per-sample rel-L2 {d.tolist()}")
    out["e2e"] = e2e
    torch.save(out, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
