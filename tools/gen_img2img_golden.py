"""Generate tests/golden/img2img_samplers.pt: the reference's own samplers run on the CPU WITH A REFERENCE (`ISampler.sample`'s
ref / ref_mask / ref_noise / start_step, samplers/schema.py:153-194: merge_ref of basic.py:16-35 in front of every ddim / basic
step, get_denoised_with_reference of k_samplers.py:185-190 inside every K evaluation) and the API's `_q_sample`
(api/multimodal/diffusion.py:1568-1613).

    python tools/gen_img2img_golden.py

Needs the reference tree (oracle/refharness finds it); writes data only.  Contents:
  * steps: {ddim eps, ddim v, basic eps, basic x0, and k_euler_a / k_heun / k_dpmpp_2m each as eps / default sigmas / float
    timesteps and v / karras / quantised} x start_step {0, 3} of 8 steps x reference {none; mask [2, 1, 3, 3]; mask [1, 4, 3, 3]}
    x guidance {off, 7.5} on a seeded [2, 4, 3, 3] state (H W = 9: a vector of four flat indices straddles channels).  For ddim /
    basic the first mask goes with a fresh draw per merge and the second with the unified reference noise.  Masks hold 0, 1 and
    the fractional values of a bilinear edge.  Recorded per run: every model output, every `torch.randn_like` draw in the order
    the reference draws them (ddim / basic: the merge's draw, where it makes one, then the step's), the timestep every `denoise`
    call received, the scalars of every row (`table`, and `side` = the q-sampler weights of every merge) formed from the
    reference's own buffers, and the SHA-256 of the f32 bytes of the image in front of the run and after every executed step;
  * q_sample: `DiffusionAPI._q_sample` called with a stand-in `self` for ddim, basic and k_euler_a over (fidelity, num_steps)
    points including fidelity 0, 1, 0.999 and `.5` rounding ties: start_step, t and the q-sampled z;
  * e2e: the reference `UNetDiffuser` with the weights of tests/golden/unet_small.pt (not stored again), 12 steps, guidance 3.0:
    per kind an image-to-image run from start_step 4 (z = `_q_sample` of a seeded reference), and for ddim, k_euler_a and
    k_dpmpp_2m an inpainting run from pure noise (half-plane mask with a fractional edge, unified reference noise), each in fp32
    and under CPU bf16 autocast with recorded noise.  Every autocast-vs-fp32 per-sample distance is asserted to be at least the
    smallest one recorded in k_samplers.pt / ddpm_samplers.pt: a 1.1 x margin on it is no tighter in absolute terms than one
    the suite already holds.
Single-threaded and seeded: a second run writes the same bytes.

As in tools/gen_k_sampler_golden.py the model outputs and the draws sit on coarse grids and are stored as int8 codes (outputs
k / 64, |k| <= 96; draws a sum of four seeded integers in [-31, 31] over 32)."""
import hashlib
import importlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from refharness import import_cflearn  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "img2img_samplers.pt")
OUTPUT_SCALE, NOISE_SCALE = 1.0 / 64, 1.0 / 32
K_COLUMNS = ("t", "sigma", "c_out", "c_skip", "c_in_next", "dt", "sigma_up", "sigma_ratio", "expm1_neg_h", "r_plus", "r_minus", "flag")
K_KINDS = ("k_euler_a", "k_heun", "k_dpmpp_2m")


def codes(ts, scale):
    """int8 codes of values on the grid `scale` (exact: checked)"""
    t = torch.stack(ts) if isinstance(ts, (list, tuple)) else ts
    q = torch.round(t / scale)
    assert q.abs().max() <= 127 and torch.equal(q * scale, t)
    return q.to(torch.int8)


def sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def rel_l2(a, f):
    return (a - f).flatten(1).norm(dim=1) / f.flatten(1).norm(dim=1)


def yardstick_floor() -> float:
    """the smallest autocast-vs-fp32 per-sample distance the existing sampler fixtures record"""
    lo = float("inf")
    for name, kinds in (("k_samplers.pt", K_KINDS), ("ddpm_samplers.pt", ("ddim", "basic"))):
        e = torch.load(os.path.join(GOLDEN, name), map_location="cpu", weights_only=False)["e2e"]
        for k in kinds:
            lo = min(lo, rel_l2(e[f"{k}_autocast"], e[f"{k}_fp32"]).min().item())
    return lo


def main() -> None:
    torch.set_num_threads(1)
    import_cflearn()
    ddpm_mod = sys.modules["cflearn.modules.multimodal.diffusion.ddpm"]
    ddim_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.samplers.ddim")
    basic_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.samplers.basic")
    schema_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.samplers.schema")
    k_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.samplers.k_samplers")
    unet_mod = importlib.import_module("cflearn.modules.multimodal.diffusion.unet")
    api_mod = importlib.import_module("cflearn.api.multimodal.diffusion")
    DDPM = ddpm_mod.DDPM
    k_classes = dict(k_euler_a=k_mod.KEulerAncestralSampler, k_heun=k_mod.KHeunSampler, k_dpmpp_2m=k_mod.KDPMpp2MSampler)

    class StandIn(torch.nn.Module):
        """exactly what the samplers read off a DDPM: the schedule buffers, t, parameterization, the v conversions, the DDPM
        q-sampler, condition_model / get_cond (identity), denoise"""

        def __init__(self, parameterization: str, schedule: str = "linear"):
            super().__init__()
            self.parameterization, self.v_posterior = parameterization, 0.0
            self.anchor = torch.nn.Parameter(torch.zeros(1))  # get_device(model)
            DDPM._register_noise_schedule(self, 1000, None, schedule, 8.5e-4, 1.2e-2, 8.0e-3)
            self.condition_model = object()
            self.get_cond = lambda c: c
            self.predict_eps_from_z_and_v = types.MethodType(DDPM.predict_eps_from_z_and_v, self)
            self.predict_start_from_z_and_v = types.MethodType(DDPM.predict_start_from_z_and_v, self)
            self.q_sampler = schema_mod.DDPMQSampler(self)
            self.q_sampler.reset_buffers(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)

    real_randn_like = torch.randn_like
    noise_gen = torch.Generator().manual_seed(380)

    def near_normal(shape):
        q = sum(torch.randint(-31, 32, shape, generator=noise_gen) for _ in range(4))
        return q.float() * NOISE_SCALE

    def make(kind, m, *, scale, uncond, eta=0.5, temperature=0.9, quantize=False, k_sched=None):
        """the reference sampler of `kind` over the stand-in `m` (guidance for `basic`, which BasicSampler does not apply itself,
        goes through UncondSamplerMixin._uncond_denoise, as in tools/gen_sampler_golden.py)"""
        gs = scale if scale is not None else 1.0
        if kind == "ddim":
            return ddim_mod.DDIMSampler(m, eta=eta, discretize="uniform", temperature=temperature, unconditional_cond=uncond,
                                        unconditional_guidance_scale=gs)
        if kind == "basic":
            if scale is not None:
                inner = m.denoise
                ns = types.SimpleNamespace(model=types.SimpleNamespace(denoise=inner), uncond=uncond, uncond_guidance_scale=scale)
                m.denoise = lambda image, ts, c, step, total, ns=ns: schema_mod.UncondSamplerMixin._uncond_denoise(
                    ns, image, ts, c, step, total)
            return basic_mod.BasicSampler(m, temperature=temperature)
        return k_classes[kind](m, default_quantize=quantize, sigmas_scheduler=k_sched, unconditional_cond=uncond,
                               unconditional_guidance_scale=gs)

    def prime(kind, s, steps, *, scale, uncond, eta=0.5, quantize=False, k_sched=None):
        """what `_q_sample` does in front of a run that starts part-way: the buffers of the run (`initialized` stays set)"""
        gs = scale if scale is not None else 1.0
        if kind == "ddim":
            s._reset_buffers(eta, "uniform", steps, uncond, gs)
        elif kind in K_KINDS:
            s._reset_buffers(steps, quantize, uncond, gs, k_sched)

    def run(sampler, z, cond, steps, *, start_step=0, ref=None, ref_mask=None, ref_noise=None, unified=False, draws_in=None):
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
            y = sampler.sample(z, ref=ref, ref_mask=ref_mask, ref_noise=ref_noise, cond=cond, num_steps=steps, start_step=start_step,
                               verbose=False, use_unified_ref_noise=unified)
        finally:
            torch.randn_like = real_randn_like
            sampler.sample_step = inner
        return y.detach().clone(), draws, images, rows

    def step_scalars(sampler, step, total):
        """ddim / basic: the scalars one step multiplies with, as the reference forms them (tools/gen_sampler_golden.py), then
        (w_net, w_noise) of the merge in front of it: the sampler's q-sampler at t_prev = total - step - 1 (basic.py:29-33)"""
        m = sampler.model
        if isinstance(sampler, ddim_mod.DDIMSampler):
            t = sampler._t
            one = lambda v: v.reshape(-1)[:1]  # noqa: E731
            at, ap, sg = one(sampler._at), one(sampler._a_prev_t), one(sampler._sigmas_t)
            vals = [torch.tensor([float(t)]), at.sqrt(), one(sampler._sqrt_one_minus_at), ap.sqrt(),
                    (1.0 - ap - sg ** 2).sqrt(), sg, m.sqrt_alphas_cumprod[t:t + 1], m.sqrt_one_minus_alphas_cumprod[t:t + 1]]
        elif isinstance(sampler, basic_mod.BasicSampler):
            t = total - step - 1
            mask = 1.0 - (torch.tensor([t]) == 0).float()
            vals = [torch.tensor([float(t)]), m.posterior_coef1[t:t + 1], m.posterior_coef2[t:t + 1],
                    mask * (0.5 * m.posterior_log_variance_clipped[t:t + 1]).exp(), torch.zeros(4)]
        else:
            return None
        q = sampler.q_sampler
        tp = total - step - 1
        return torch.cat(vals + [q.sqrt_alphas[tp:tp + 1].float(), q.sqrt_one_minus_alphas[tp:tp + 1].float()])

    def k_scalars(kind, par, s, steps, quantize, start_step):
        """one row per model evaluation of the FULL run, from the reference's buffers and expressions (tools/gen_k_sampler_golden.py);
        k_dpmpp_2m: the step the run starts at has `old_denoised is None`, flag 0"""
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
                up = (torch.ones(1) * 1.0 * sigma_up)[0]
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
                if step == 0 or step == start_step:
                    rp, rm, flag = zero, zero, zero
                else:
                    h_last = t - s.t_fn(s.sigmas[step - 1])
                    r = h_last / h
                    rp, rm, flag = 1 + 1 / (2 * r), 1 / (2 * r), one
                rows.append(head(step, step + 1) + [zero, zero, ratio, em1, rp, rm, flag])
        return torch.stack([torch.stack([v.float().reshape(()) for v in r]) for r in rows])

    out: dict = {"steps": [], "q_sample": [], "e2e": {}, "k_columns": K_COLUMNS}
    # ---- step records
    torch.manual_seed(350)
    z = torch.randn(2, 4, 3, 3)
    ref = torch.randn(2, 4, 3, 3)
    ref_noise = near_normal((2, 4, 3, 3))
    cond = torch.randn(2, 4, 8)
    uncond = torch.randn(1, 4, 8)
    edge = torch.tensor([1.0, 0.625, 0.0])  # a bilinear edge between kept and free
    masks = {
        "b1": torch.stack([edge.repeat(3, 1), torch.tensor([[0.0, 0.25, 1.0], [1.0, 1.0, 0.0], [0.75, 0.0, 0.0]])]).view(2, 1, 3, 3),
        "1c": torch.stack([edge.repeat(3, 1), edge.repeat(3, 1).t().contiguous(), torch.ones(3, 3), torch.zeros(3, 3)]).view(1, 4, 3, 3),
    }
    out.update(step_z=z.clone(), step_ref=ref.clone(), step_ref_noise=ref_noise.clone(), step_cond=cond.clone(),
               step_uncond=uncond.clone(), step_masks={k: v.clone() for k, v in masks.items()})
    specs = [("ddim", "eps", "linear", None, False), ("ddim", "v", "cosine", None, False), ("basic", "eps", "linear", None, False),
             ("basic", "x0", "linear", None, False)]
    for kind in K_KINDS:
        specs += [(kind, "eps", "linear", None, False), (kind, "v", "linear", "karras", True)]
    steps, ci = 8, 0
    for kind, par, sched, k_sched, quantize in specs:
        is_k = kind in K_KINDS
        for start_step in (0, 3):
            for mask_name in (None, "b1", "1c"):
                unified = (not is_k) and mask_name == "1c"
                for scale in (None, 7.5):
                    m = StandIn(par, sched)
                    gen = torch.Generator().manual_seed(400 + ci)
                    ci += 1
                    outputs, seen_ts = [], []

                    def raw(image, ts, c, step, total, gen=gen, outputs=outputs, seen_ts=seen_ts):
                        o = torch.randint(-96, 97, image.shape, generator=gen).float() * OUTPUT_SCALE
                        outputs.append(o.clone())
                        seen_ts.append(ts.clone())
                        return o

                    m.denoise = raw
                    s = make(kind, m, scale=scale, uncond=uncond, quantize=quantize, k_sched=k_sched)
                    if start_step > 0:
                        prime(kind, s, steps, scale=scale, uncond=uncond, quantize=quantize, k_sched=k_sched)
                    kw = {}
                    if mask_name is not None:
                        kw = dict(ref=ref, ref_mask=masks[mask_name], ref_noise=ref_noise if unified else None, unified=unified)
                    y, draws, images, rows = run(s, z, cond if scale is not None else None, steps, start_step=start_step, **kw)
                    assert torch.equal(y, images[-1]) and torch.equal(images[0], z) and len(images) == steps - start_step + 1
                    assert all(bool((t == t[0]).all()) for t in seen_ts)
                    tss = torch.stack([t[0] for t in seen_ts])
                    rec = dict(kind=kind, parameterization=par, schedule=sched, sigmas_scheduler=k_sched, quantize=quantize, scale=scale,
                               steps=steps, start_step=start_step, mask=mask_name, unified=unified, eta=0.5 if kind == "ddim" else 0.0,
                               discretize="uniform", temperature=0.9, outputs_q=codes(outputs, OUTPUT_SCALE), outputs_scale=OUTPUT_SCALE,
                               timesteps=tss, image_sha256=[sha(im) for im in images])
                    if is_k:
                        s._reset_buffers(steps, quantize, None, 1.0, k_sched)  # (sample() leaves the buffers; rebuilt for the scalars)
                        table = k_scalars(kind, par, s, steps, quantize, start_step)
                        per = 2 if kind == "k_heun" else 1
                        assert table.shape[0] - start_step * per == len(outputs)
                        assert torch.equal(tss.float(), table[start_step * per:, 0])
                        rec.update(table=table, sigmas=s.sigmas.clone())
                        assert len(draws) == {"k_euler_a": steps - 1 - start_step, "k_heun": steps - 1 - start_step, "k_dpmpp_2m": 0}[kind]
                    else:
                        rows = torch.stack(rows)
                        assert rows.shape == (steps - start_step, 10) and torch.equal(tss.float(), rows[:, 0])
                        rec.update(table=rows[:, :8].clone(), side=rows[:, 8:].clone())
                        merges = steps - start_step if (mask_name is not None and not unified) else 0
                        assert len(draws) == steps - start_step + merges
                    if draws:
                        rec.update(draws_q=codes(draws, NOISE_SCALE), draws_scale=NOISE_SCALE)
                    out["steps"].append(rec)

    # ---- DiffusionAPI._q_sample with a stand-in `self`
    torch.manual_seed(360)
    qz = torch.randn(2, 4, 3, 3)
    qn = near_normal((2, 4, 3, 3))
    out.update(q_z=qz.clone(), q_noise=qn.clone())
    for kind in ("ddim", "basic", "k_euler_a"):
        for fidelity, n in ((0.0, 8), (1.0, 8), (0.999, 8), (0.5, 8), (0.5, 10), (0.5, 11), (0.2, 50), (0.8, 25), (0.3, 12), (0.4, 12)):
            m = StandIn("eps")
            s = make(kind, m, scale=None, uncond=None, eta=0.0, temperature=1.0)
            api = types.SimpleNamespace(m=types.SimpleNamespace(sampler=s), _random_state=None)
            zq, noise, start_step = api_mod.DiffusionAPI._q_sample(api, qz, n, fidelity, 0, q_sample_noise=qn)
            assert torch.equal(noise, qn)
            t = n - start_step - 1 if kind in K_KINDS else n - start_step
            out["q_sample"].append(dict(kind=kind, fidelity=fidelity, num_steps=n, t=int(t), start_step=int(start_step), z=zq.clone()))

    # ---- end to end on the small UNet fixture
    u = torch.load(os.path.join(GOLDEN, "unet_small.pt"), map_location="cpu", weights_only=False)
    net = unet_mod.UNetDiffuser(**u["cfg"])
    net.load_state_dict(u["sd"])
    net.eval()
    torch.manual_seed(370)
    z_ref = torch.tanh(torch.randn(2, 3, 16, 16))
    start_noise = near_normal((2, 3, 16, 16))
    cond = torch.randn(2, 5, 48)
    uncond = torch.randn(1, 5, 48)
    col = torch.zeros(16)
    col[:7], col[7] = 1.0, 0.5
    mask = col.repeat(16, 1).view(1, 1, 16, 16).contiguous()  # the left half keeps the reference; one fractional column
    n_steps, gs = 12, 3.0
    e2e = dict(z_ref=z_ref, start_noise=start_noise, cond=cond, uncond=uncond, steps=n_steps, scale=gs, mask=mask,
               fidelity=dict(ddim=0.3, basic=0.3, k_euler_a=0.4, k_heun=0.4, k_dpmpp_2m=0.4), runs={})
    floor = yardstick_floor()
    print(f"yardstick floor (smallest recorded autocast-vs-fp32 distance): {floor:.6g}")
    net_denoise = lambda image, ts, c, step, total: net(image, timesteps=ts, context=c)  # noqa: E731

    def e2e_sampler(kind):
        m = StandIn("eps")
        if kind == "basic":  # (BasicSampler applies no guidance: the context goes in directly, as in tools/gen_sampler_golden.py)
            m.denoise = lambda image, ts, c, step, total: net(image, timesteps=ts, context=cond)
            return make(kind, m, scale=None, uncond=None, temperature=1.0)
        m.denoise = net_denoise
        return make(kind, m, scale=gs, uncond=uncond, eta=0.0, temperature=1.0)

    with torch.no_grad():
        for kind in ("ddim", "basic") + K_KINDS:
            jobs = [("img2img", e2e["fidelity"][kind])]
            if kind in ("ddim", "k_euler_a", "k_dpmpp_2m"):
                jobs.append(("inpaint", None))
            for job, fidelity in jobs:
                if job == "img2img":
                    s = e2e_sampler(kind)
                    api = types.SimpleNamespace(m=types.SimpleNamespace(sampler=s), _random_state=None)
                    z0, _, start_step = api_mod.DiffusionAPI._q_sample(api, z_ref, n_steps, fidelity, 0, q_sample_noise=start_noise)
                    assert start_step == 4
                    kw = dict(start_step=start_step)
                else:
                    z0, start_step = start_noise, 0
                    kw = dict(ref=z_ref, ref_mask=mask, ref_noise=start_noise, unified=True)
                res = {}
                draws = None
                for form in ("fp32", "autocast"):
                    s = e2e_sampler(kind)
                    if start_step > 0:
                        prime(kind, s, n_steps, scale=gs, uncond=uncond, eta=0.0)
                    if form == "fp32":
                        y, draws, _, _ = run(s, z0, None if kind == "basic" else cond, n_steps, **kw)
                    else:
                        with torch.autocast("cpu", dtype=torch.bfloat16):
                            y = run(s, z0, None if kind == "basic" else cond, n_steps, draws_in=draws, **kw)[0].float()
                    assert torch.isfinite(y).all()
                    res[form] = y
                d = rel_l2(res["autocast"], res["fp32"])
                print(f"{kind} {job}: bf16-autocast vs fp32 per-sample rel-L2 {d.tolist()}")
                assert d.min().item() >= floor, f"{kind} {job}: the yardstick {d.tolist()} collapsed below {floor}: change the mask"
                rec = dict(start_step=start_step, z=z0.clone(), fp32=res["fp32"], autocast=res["autocast"])
                if draws and kind in ("basic", "k_euler_a"):  # (ddim runs at eta 0 and k_heun never uses its draw: not recorded)
                    rec.update(noise_q=codes(draws, NOISE_SCALE), noise_scale=NOISE_SCALE)
                e2e["runs"][f"{kind}_{job}"] = rec
    out["e2e"] = e2e
    torch.save(out, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
