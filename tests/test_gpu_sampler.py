"""DDIM / ancestral sampling on the GPU (csrc/sample.hip, diffusion.make_sampler) against the reference's own samplers
(tests/golden/ddpm_samplers.pt, tools/gen_sampler_golden.py): the fused step kernel teacher-forced and free-running on the
recorded model outputs and noises, the Philox normal generator, end-to-end sampling with the small UNet against the
reference's fp32 run with its bf16-autocast distance as the yardstick, graph == eager, the frozen filter packs, and a
guided graph run of the zoo-size UNet."""
import math

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import functional as HF
from cflearn_amd import ops
from cflearn_amd.diffusion import NoiseSchedule, make_sampler, sampler_table
from sampler_replay import decode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ddpm_samplers.pt")


@pytest.fixture(scope="module")
def small(golden):
    u = golden("unet_small.pt")
    m = C.build_module("unet_diffuser", config=dict(u["cfg"]))
    m.load_state_dict(u["sd"])
    return m.to(DEV)


def _outs(r, d, k):
    b = d["images"].shape[1]
    o = d["outputs"][k].to(DEV).bfloat16()
    assert torch.equal(o.float().cpu(), d["outputs"][k])  # the recorded outputs are bf16 values
    return (o, None) if r["scale"] is None else (o[:b].contiguous(), o[b:].contiguous())


def test_step_kernel_teacher_forced_matches_the_reference(fx):
    """every recorded step of every sampler x guidance case: the reference's input image, model output(s) and noise in,
    the reference's scalars of the step (recorded: a host's own transcendental functions may differ in the last bit), the
    reference's next image out within 4 f32 ulps of each element's magnitude; the bf16 UNet input is the rounded state"""
    assert len(fx["steps"]) == 8
    for r in fx["steps"]:
        d = decode(fx, r)
        table, bank = d["table"].to(DEV), d["noises"].to(DEV).contiguous()
        for k in range(r["steps"]):
            x = d["images"][k].to(DEV).contiguous().clone()
            xin = torch.empty((2,) + tuple(x.shape), dtype=torch.bfloat16, device=DEV).view(-1, *x.shape[1:])
            oc, ou = _outs(r, d, k)
            kt = torch.tensor([k], dtype=torch.int32, device=DEV)
            ops.diffusion_sample_step(x, xin, oc, table, kt, kind=r["kind"], parameterization=r["parameterization"], out_u=ou,
                                      scale=r["scale"] or 1.0, noise=bank, temperature=r["temperature"])
            want = d["images"][k + 1]
            err = (x.cpu() - want).abs()
            tol = 4 * F32_EPS * want.abs()
            assert bool((err <= tol).all()), (r["kind"], r["parameterization"], r["scale"], k, err.max().item())
            b = x.shape[0]
            assert torch.equal(xin[:b].cpu(), x.cpu().bfloat16()) and torch.equal(xin[b:].cpu(), x.cpu().bfloat16())


def test_step_kernel_free_run_on_the_recorded_outputs(fx):
    """all steps chained on the device (advance bumps k and the timesteps) from z: every intermediate image within 1e-5"""
    for r in fx["steps"]:
        d = decode(fx, r)
        table, bank = d["table"].to(DEV), d["noises"].to(DEV).contiguous()
        x = d["images"][0].to(DEV).contiguous().clone()
        xin = torch.empty_like(x, dtype=torch.bfloat16)
        k = torch.zeros((1,), dtype=torch.int32, device=DEV)
        ts = torch.full((x.shape[0],), -1, dtype=torch.int64, device=DEV)
        worst = 0.0
        for step in range(r["steps"]):
            oc, ou = _outs(r, d, step)
            ops.diffusion_sample_step(x, xin, oc, table, k, kind=r["kind"], parameterization=r["parameterization"], out_u=ou,
                                      scale=r["scale"] or 1.0, noise=bank, temperature=r["temperature"])
            ops.diffusion_sample_advance(k, table, ts)
            want = d["images"][step + 1]
            worst = max(worst, ((x.cpu() - want).norm() / want.norm()).item())
            if step + 1 < r["steps"]:
                assert ts.cpu().tolist() == [int(table[step + 1, 0].item())] * x.shape[0]
        assert k.item() == r["steps"]
        assert worst <= 1e-5, (r["kind"], r["parameterization"], r["scale"], worst)


def test_philox_normal_statistics_and_reproducibility():
    n = 1 << 22
    z = ops.randn(n, 1234, 0, DEV)
    zd = z.double().cpu()
    mean, var = zd.mean().item(), zd.var().item()
    kurt = (((zd - mean) ** 4).mean() / var ** 2).item()
    assert abs(mean) < 5 / math.sqrt(n), mean
    assert abs(var - 1) < 5 * math.sqrt(2 / n), var
    assert abs(kurt - 3) < 5 * math.sqrt(24 / n), kurt
    s, _ = zd.sort()
    cdf = torch.special.ndtr(s)
    i = torch.arange(1, n + 1, dtype=torch.float64)
    ks = torch.maximum(i / n - cdf, cdf - (i - 1) / n).max().item()
    assert ks < 1.9495 / math.sqrt(n), ks  # Kolmogorov critical value at 1e-3
    assert torch.isfinite(z).all()
    assert torch.equal(ops.randn(n, 1234, 0, DEV), z)  # same (seed, offset): same bits
    assert torch.equal(ops.randn(n - 4, 1234, 1, DEV), z[4:])  # counter = offset + i / 4
    assert not torch.equal(ops.randn(1024, 1235, 0, DEV), z[:1024])
    # the step kernel's own draws: basic / x0 with zero model output and a unit noise scale writes xi itself
    b, shape = 4, (3, 32, 32)
    nel = int(torch.tensor(shape).prod())
    table = torch.zeros((2, ops.SAMPLE_ROW), dtype=torch.float32)
    table[:, 3] = 1.0
    table = table.to(DEV)
    zero = torch.zeros((b, *shape), dtype=torch.bfloat16, device=DEV)
    draws = []
    for k in range(2):
        x = torch.zeros((b, *shape), device=DEV)
        ops.diffusion_sample_step(x, torch.empty_like(zero), zero, table, torch.tensor([k], dtype=torch.int32, device=DEV),
                                  kind="basic", parameterization="x0", seed=77, offset=b * nel // 4)
        draws.append(x.flatten(1).double().cpu())
        assert torch.equal(x.flatten(), ops.randn(b * nel, 77, (1 + k) * b * nel // 4, DEV))
    bound = 5 / math.sqrt(nel)
    for k in range(2):  # samples of one step
        c = torch.corrcoef(draws[k])
        assert (c - torch.eye(b, dtype=torch.float64)).abs().max().item() < bound
    c = torch.corrcoef(torch.cat([draws[0], draws[1]]))[:b, b:]  # steps
    assert c.abs().max().item() < bound


def _per_sample(a, ref):
    a, ref = a.float().cpu().flatten(1), ref.float().flatten(1)
    return ((a - ref).norm(dim=1) / ref.norm(dim=1)).tolist()


def test_ddim_end_to_end_small_unet_within_the_reference_bf16_distance(fx, small):
    e = fx["e2e"]
    s = make_sampler("ddim", small, NoiseSchedule(device=DEV), eta=0.0, unconditional_cond=e["uncond"],
                     unconditional_guidance_scale=e["scale"])
    y = s.sample(e["z"].to(DEV), cond=e["cond"].to(DEV), num_steps=e["steps"], clip_output=False)
    mine, yard = _per_sample(y, e["ddim_fp32"]), _per_sample(e["ddim_autocast"], e["ddim_fp32"])
    print(f"ddim e2e per-sample rel-L2 vs fp32: HIP {mine}, reference bf16 autocast {yard}")
    for a, b in zip(mine, yard):
        assert a <= 1.1 * b, (mine, yard)
    yc = s.sample(e["z"].to(DEV), cond=e["cond"].to(DEV), num_steps=e["steps"])  # clip_output=True: the last step clamps
    assert torch.equal(yc, y.clamp(-1.0, 1.0))


def test_basic_end_to_end_small_unet_with_recorded_noise(fx, small):
    e = fx["e2e"]
    s = make_sampler("basic", small, NoiseSchedule(device=DEV))
    y = s.sample(e["z"].to(DEV), cond=e["cond"].to(DEV), num_steps=e["steps"],
                 noise=e["basic_noise_q"].float() * e["basic_noise_scale"], clip_output=False)
    mine, yard = _per_sample(y, e["basic_fp32"]), _per_sample(e["basic_autocast"], e["basic_fp32"])
    print(f"basic e2e per-sample rel-L2 vs fp32: HIP {mine}, reference bf16 autocast {yard}")
    for a, b in zip(mine, yard):
        assert a <= 1.1 * b, (mine, yard)


@pytest.mark.parametrize("guided", [False, True])
def test_graph_equals_eager_bit_for_bit(fx, small, guided):
    e = fx["e2e"]
    cfg = dict(eta=0.5) if not guided else dict(eta=0.5, unconditional_cond=e["uncond"], unconditional_guidance_scale=3.0)
    s = make_sampler("ddim", small, NoiseSchedule(device=DEV), **cfg)
    kw = dict(num_samples=2, shape=(3, 16, 16), cond=e["cond"].to(DEV), num_steps=8, seed=5)
    eager = s.sample(**kw)
    graph = s.sample(**kw, use_graph=True)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph), (eager - graph).abs().max().item()
    assert not torch.equal(s.sample(**dict(kw, seed=6)), eager)


def test_frozen_conv_packs_forward_is_bit_identical_and_packs_no_rotated_matrix(small, monkeypatch):
    torch.manual_seed(3)
    x = torch.randn(2, 3, 16, 16).to(DEV)
    t = torch.tensor([5, 700], device=DEV)
    ctx = torch.randn(2, 5, 48).to(DEV)
    with torch.no_grad():
        want = small(x, timesteps=t, context=ctx)
        rotated = []
        real_grouped, real_single = ops.conv3x3_pack_grouped, ops.conv3x3_pack_filters
        monkeypatch.setattr(ops, "conv3x3_pack_grouped", lambda items: (rotated.extend(r for _, _, r in items), real_grouped(items))[1])
        monkeypatch.setattr(ops, "conv3x3_pack_filters", lambda w, rot, **k: (rotated.append(rot), real_single(w, rot, **k))[1])
        with HF.frozen_conv_packs(small) as packs:
            assert len(packs) == len(small._packable_convs()) > 0
            assert all(r is None for _, r in packs.values())
            n_entry = len(rotated)
            got = [small(x, timesteps=t, context=ctx) for _ in range(2)]
            # inside a forward only the 3-channel head (zero-padded filters, not a packable conv) still packs its own matrix
            assert len(rotated) - n_entry <= 2
        assert HF.frozen_packs_of(small) is None
        assert not any(rotated), "a rotated (dX) filter matrix was packed"
    for g in got:
        assert torch.equal(g, want)


def test_zoo_unet_guided_graph_sampling():
    """the zoo diffusion/ddpm UNet (with a 768-wide context for the guidance) at 64^2 x 8: 10 guided DDIM steps (a
    16-sample forward each) as a replayed graph.  Its head is zero-initialised, so the model output is small after a small
    perturbation and the DDIM state grows like z * sqrt(a_prev) / sqrt(a_t) over the run; the state's std over that
    factor must stay in [0.5, 2], and everything finite."""
    torch.manual_seed(0)
    cfg = dict(in_channels=3, out_channels=3, start_channels=320, num_heads=8, use_spatial_transformer=True,
               num_transformer_layers=1, num_res_blocks=2, attention_downsample_rates=(1, 2, 4),
               channel_multipliers=(1, 2, 4, 4), context_dim=768)
    m = C.build_module("unet_diffuser", config=cfg).to(DEV)
    with torch.no_grad():
        for p in m.head[2].parameters():
            p.normal_(0.0, 1e-3)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(8, 77, 768, generator=g).to(DEV)
    uncond = torch.randn(1, 77, 768, generator=g)
    sched = NoiseSchedule(device=DEV)
    s = make_sampler("ddim", m, sched, unconditional_cond=uncond, unconditional_guidance_scale=7.5)
    y = s.sample(num_samples=8, shape=(3, 64, 64), cond=cond, num_steps=10, seed=11, clip_output=False, use_graph=True)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    tb = sampler_table("ddim", sched, 10)
    growth = 1.0
    for k in range(10):
        growth *= (tb[k, 3] / tb[k, 1]).item()
    ratio = y.std().item() / growth
    print(f"zoo UNet guided graph sampling: std {y.std().item():.4f}, DDIM growth {growth:.4f}, ratio {ratio:.4f}")
    assert 0.5 <= ratio <= 2.0, ratio
