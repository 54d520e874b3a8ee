"""Generate tests/golden/ddpm_samplers.pt: the reference's own DDIM and ancestral ("basic") samplers run on the CPU.

    python tools/gen_sampler_golden.py

Needs the reference tree (oracle/refharness finds it); writes data only.  Contents:
  * tables: `DDIMMixin._reset_buffers` (ddim.py:241-268, through `DDIMQSampler.reset_buffers`, ddim.py:37-53) for
    {linear, cosine} x {uniform, quad} x {10, 50} steps x eta {0, 0.5}, and the posterior buffers of
    `DDPM._register_noise_schedule` (ddpm.py:599-650) the basic sampler reads;
  * steps: {ddim eps, ddim v, basic eps, basic x0} x guidance {off, 7.5} on a seeded [2, 3, 16, 16] state, the reference's
    `ISampler.sample` over a stand-in model whose `denoise` returns seeded bf16-representable outputs; every model output,
    every `torch.randn_like` draw and every intermediate image is recorded (guidance for `basic`, which the reference's
    BasicSampler does not apply itself, goes through `UncondSamplerMixin._uncond_denoise`);
  * e2e: the reference `UNetDiffuser` with the weights of tests/golden/unet_small.pt (not stored again): DDIM eta 0, 20
    steps, guidance 3.0 with an unconditional context, in fp32 and under CPU bf16 autocast (the reference's own
    mixed-precision distance); basic 20 steps with recorded noise, the same two forms.
Single-threaded and seeded: a second run writes the same bytes.

To keep the file small the model outputs and the noise are drawn on coarse grids and stored as int8 codes: outputs are
k / 64 (|k| <= 96, exact in bf16), and `torch.randn_like` is replaced by a recorded near-normal draw (a sum of four seeded
integers in [-31, 31], over 32: std ~1.14, exact in f32).  Decode a code tensor q as q.float() * <name>_scale.  The
intermediate images of the step records are not stored: each step's SHA-256 (of the f32 bytes) is, together with the
scalars of each step as the reference formed them (`table`); the tests rebuild the chain from `step_z` with the kernel's
operation order in numpy f32 (one IEEE rounding per operation on every host) and check every image against it."""
import hashlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from refharness import import_cflearn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ddpm_samplers.pt")
OUTPUT_SCALE, NOISE_SCALE = 1.0 / 64, 1.0 / 32


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
    import importlib

    ddim_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.samplers.ddim")
    basic_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.samplers.basic")
    schema_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.samplers.schema")
    unet_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.unet")
    DDPM = ddpm_mod.DDPM

    class StandIn(torch.nn.Module):
        """exactly what the samplers read off a DDPM: the schedule buffers, t, parameterization, the v conversions,
        condition_model / get_cond (identity), denoise"""

        def __init__(self, parameterization: str, schedule: str):
            super().__init__()
            self.parameterization, self.v_posterior = parameterization, 0.0
            self.anchor = torch.nn.Parameter(torch.zeros(1))  # get_device(model)
            DDPM._register_noise_schedule(self, 1000, None, schedule, 8.5e-4, 1.2e-2, 8.0e-3)
            self.condition_model = object()
            self.get_cond = lambda c: c
            self.predict_eps_from_z_and_v = types.MethodType(DDPM.predict_eps_from_z_and_v, self)
            self.predict_start_from_z_and_v = types.MethodType(DDPM.predict_start_from_z_and_v, self)

    out: dict = {"tables": {"ddim": [], "posterior": {}}, "steps": [], "e2e": {}}
    # ---- tables
    for sched in ("linear", "cosine"):
        m = StandIn("eps", sched)
        out["tables"]["posterior"][sched] = dict(
            alphas_cumprod=m.alphas_cumprod.clone(), alphas_cumprod_prev=m.alphas_cumprod_prev.clone(),
            posterior_log_variance_clipped=m.posterior_log_variance_clipped.clone(),
            posterior_coef1=m.posterior_coef1.clone(), posterior_coef2=m.posterior_coef2.clone())
        for disc in ("uniform", "quad"):
            for steps in (10, 50):
                for eta in (0.0, 0.5):
                    s = ddim_mod.DDIMSampler(m, eta=eta, discretize=disc)
                    s._reset_buffers(eta, disc, steps, None, 1.0)
                    out["tables"]["ddim"].append(dict(
                        schedule=sched, discretize=disc, steps=steps, eta=eta, timesteps=list(s.ddim_timesteps),
                        alphas=s.ddim_alphas.clone(), alphas_prev=s.ddim_alphas_prev.clone(), sigmas=s.ddim_sigmas.clone(),
                        sqrt_one_minus_alphas=s.ddim_sqrt_one_minus_alphas.clone()))

    real_randn_like = torch.randn_like
    noise_gen = torch.Generator().manual_seed(180)

    def near_normal(shape):
        q = sum(torch.randint(-31, 32, shape, generator=noise_gen) for _ in range(4))
        return q.float() * NOISE_SCALE

    def run(sampler, z, cond, steps, draws_in=None):
        """sampler.sample with every randn_like draw (a recorded near-normal one) and every step's image recorded (or the
        draws replayed)"""
        draws, images, rows = [], [z.clone()], []
        it = iter(draws_in) if draws_in is not None else None

        def randn_like(t, *a, **k):
            v = next(it).to(t.dtype) if it is not None else near_normal(t.shape).to(t.dtype)
            draws.append(v.clone())
            return v

        inner = sampler.sample_step

        def step(image, c, step_, total, *a, **k):
            r = inner(image, c, step_, total, *a, **k)
            images.append(r.detach().clone())
            rows.append(step_scalars(sampler, step_, total))
            return r

        sampler.sample_step = step
        torch.randn_like = randn_like
        try:
            y = sampler.sample(z, cond=cond, num_steps=steps, verbose=False)
        finally:
            torch.randn_like = real_randn_like
        return y.detach().clone(), draws, images, torch.stack(rows)

    def step_scalars(sampler, step, total):
        """the scalars one step of the reference multiplies with, as the reference forms them (ddim.py:167-181,
        221-239, ddpm.py:461-484, basic.py:70-92): t, then for DDIM sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev),
        sqrt(1 - a_prev - sigma^2), sigma, sqrt(ac[t]), sqrt(1 - ac[t]); for basic coef1[t], coef2[t],
        [t > 0] exp(0.5 log_var[t])"""
        m = sampler.model
        if isinstance(sampler, ddim_mod.DDIMSampler):
            t = sampler._t
            one = lambda v: v.reshape(-1)[:1]  # noqa: E731
            at, ap, sg = one(sampler._at), one(sampler._a_prev_t), one(sampler._sigmas_t)
            vals = [torch.tensor([float(t)]), at.sqrt(), one(sampler._sqrt_one_minus_at), ap.sqrt(),
                    (1.0 - ap - sg ** 2).sqrt(), sg, m.sqrt_alphas_cumprod[t:t + 1], m.sqrt_one_minus_alphas_cumprod[t:t + 1]]
        else:
            t = total - step - 1
            mask = 1.0 - (torch.tensor([t]) == 0).float()
            vals = [torch.tensor([float(t)]), m.posterior_coef1[t:t + 1], m.posterior_coef2[t:t + 1],
                    mask * (0.5 * m.posterior_log_variance_clipped[t:t + 1]).exp(), torch.zeros(4)]
        return torch.cat(vals)

    # ---- step records
    torch.manual_seed(150)
    z = torch.randn(2, 3, 16, 16)
    cond = torch.randn(2, 4, 8)
    uncond = torch.randn(1, 4, 8)
    for ci, (kind, par, sched) in enumerate((("ddim", "eps", "linear"), ("ddim", "v", "cosine"), ("basic", "eps", "linear"),
                                              ("basic", "x0", "linear"))):
        for scale in (None, 7.5):
            m = StandIn(par, sched)
            gen = torch.Generator().manual_seed(160 + 2 * ci + (scale is not None))
            outputs = []

            def raw(image, ts, c, step, total, gen=gen, outputs=outputs):
                o = torch.randint(-96, 97, image.shape, generator=gen).float() * OUTPUT_SCALE
                outputs.append(o.clone())
                return o

            steps = 8
            if kind == "ddim":
                m.denoise = raw
                s = ddim_mod.DDIMSampler(m, eta=0.5, discretize="uniform", temperature=0.9, unconditional_cond=uncond,
                                         unconditional_guidance_scale=scale if scale is not None else 1.0)
            else:
                if scale is None:
                    m.denoise = raw
                else:
                    ns = types.SimpleNamespace(model=types.SimpleNamespace(denoise=raw), uncond=uncond, uncond_guidance_scale=scale)
                    m.denoise = lambda image, ts, c, step, total, ns=ns: schema_mod.UncondSamplerMixin._uncond_denoise(
                        ns, image, ts, c, step, total)
                s = basic_mod.BasicSampler(m, temperature=0.9)
            y, draws, images, rows = run(s, z, cond if scale is not None else None, steps)
            assert torch.equal(y, images[-1]) and torch.equal(images[0], z)
            out["steps"].append(dict(kind=kind, parameterization=par, schedule=sched, scale=scale, steps=steps,
                                     eta=0.5 if kind == "ddim" else 0.0, discretize="uniform", temperature=0.9,
                                     cond=cond.clone(), uncond=uncond.clone(), outputs_q=codes(outputs, OUTPUT_SCALE),
                                     outputs_scale=OUTPUT_SCALE, noises_q=codes(draws, NOISE_SCALE), noises_scale=NOISE_SCALE,
                                     table=rows, image_sha256=[hashlib.sha256(im.contiguous().numpy().tobytes()).hexdigest()
                                                   for im in images]))
    out["step_z"] = z.clone()
    # ---- end to end on the small UNet fixture
    u = torch.load(os.path.join(ROOT, "tests", "golden", "unet_small.pt"), map_location="cpu", weights_only=False)
    net = unet_mod.UNetDiffuser(**u["cfg"])
    net.load_state_dict(u["sd"])
    net.eval()
    torch.manual_seed(170)
    z = torch.randn(2, 3, 16, 16)
    cond = torch.randn(2, 5, 48)
    uncond = torch.randn(1, 5, 48)
    m = StandIn("eps", "linear")
    m.denoise = lambda image, ts, c, step, total: net(image, timesteps=ts, context=c)
    e2e = dict(z=z, cond=cond, uncond=uncond, steps=20, scale=3.0)
    with torch.no_grad():
        s = ddim_mod.DDIMSampler(m, eta=0.0, unconditional_cond=uncond, unconditional_guidance_scale=3.0)
        e2e["ddim_fp32"] = run(s, z, cond, 20)[0]
        with torch.autocast("cpu", dtype=torch.bfloat16):
            s = ddim_mod.DDIMSampler(m, eta=0.0, unconditional_cond=uncond, unconditional_guidance_scale=3.0)
            e2e["ddim_autocast"] = run(s, z, cond, 20)[0].float()
        m.denoise = lambda image, ts, c, step, total: net(image, timesteps=ts, context=cond)
        y, draws, _, _ = run(basic_mod.BasicSampler(m), z, None, 20)
        e2e["basic_fp32"], e2e["basic_noise_q"], e2e["basic_noise_scale"] = y, codes(draws, NOISE_SCALE), NOISE_SCALE
        with torch.autocast("cpu", dtype=torch.bfloat16):
            e2e["basic_autocast"] = run(basic_mod.BasicSampler(m), z, None, 20, draws_in=draws)[0].float()
    out["e2e"] = e2e
    for k in ("ddim", "basic"):
        d = (e2e[f"{k}_autocast"] - e2e[f"{k}_fp32"]).flatten(1).norm(dim=1) / e2e[f"{k}_fp32"].flatten(1).norm(dim=1)
        print(f"{k}: bf16-autocast vs fp32 per-sample rel-L2 {d.tolist()}")
    torch.save(out, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
