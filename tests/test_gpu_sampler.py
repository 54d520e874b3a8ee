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
from helpers import assert_elementwise, guarded_ops
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


# ---------------------------------------------------------------------------------------------
# the step kernel per element at its edges: an f32 CPU replica (bit-equal) and the same formulas in float64
# ---------------------------------------------------------------------------------------------

BF16, F32 = torch.bfloat16, torch.float32
STEP_GROUPS = 2048 * 256  # groups of 4 elements one pass of sample_step_kernel's stride loop covers
STEP_SHAPES = [(1, 4), (3, 4), (1, 1028), (2, 4 * (STEP_GROUPS // 2 + 2))]  # the last: 524 292 groups, a second pass
STEP_FORMS = [("ddim", "eps"), ("ddim", "v"), ("basic", "eps"), ("basic", "x0")]  # every defined kind x parameterization
TEMPERATURE, GUIDANCE = 0.7, 3.0


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


def _step_table():
    """3 rows: a timestep and seven coefficients in [0.2, 1.5]"""
    t = torch.rand((3, ops.SAMPLE_ROW), generator=torch.Generator().manual_seed(11)) * 1.3 + 0.2
    t[:, 0] = torch.tensor([900.0, 500.0, 100.0])
    return t


def _step_replica(x, oc, ou, row, xi, kind, param, clamp, dtype):
    """sample_step_kernel's documented operation order with torch CPU ops in `dtype`, one rounding per operation and no
    FMA (every line below is one torch op on materialised operands) -> (next x, cond): cond is the same formula on
    absolute values, divided by |c1| where the formula divides"""
    x, m = x.to(dtype), oc.to(dtype)
    c1, c2, c3, c4, c5, c6, c7 = (row[i].to(dtype) for i in range(1, 8))
    scale, temp = torch.tensor(GUIDANCE, dtype=F32).to(dtype), torch.tensor(TEMPERATURE, dtype=F32).to(dtype)
    xi = xi.to(dtype)
    am = m.abs()
    if ou is not None:  # u + scale * (m - u)
        u = ou.to(dtype)
        d = m - u
        d = scale * d
        m = u + d
        am = u.abs() + scale * (am + u.abs())
    ax, axi = x.abs(), xi.abs()
    if kind == "ddim":
        if param == "v":
            eps = c6 * m + c7 * x
            x0 = c6 * x - c7 * m
            aeps = ax0 = c6 * am + c7 * ax
        else:
            eps = m
            t = c2 * eps
            t = x - t
            x0 = t / c1
            aeps, ax0 = am, (ax + c2 * am) / c1
        a = c3 * x0
        b = c4 * eps
        v = a + b
        nz = c5 * xi
        nz = nz * temp
        v = v + nz
        cond = c3 * ax0 + c4 * aeps + c5 * axi * temp
    else:
        nz = xi * temp
        nz = c3 * nz
        if param == "x0":
            v = m + nz
            cond = am + c3 * axi * temp
        else:
            t = c2 * m
            t = x - t
            t = c1 * t
            v = t + nz
            cond = c1 * (ax + c2 * am) + c3 * axi * temp
    return (v.clamp(-1.0, 1.0) if clamp else v), cond


def _step_inputs(b, n, guided):
    g = torch.Generator().manual_seed(1000 * b + n)
    x = torch.randn((b, n), generator=g) * 1.5
    oc = torch.randn((b, n), generator=g).to(BF16)
    ou = torch.randn((b, n), generator=g).to(BF16) if guided else None
    bank = torch.randn((3, b, n), generator=g)
    return x, oc, ou, bank


def _run_step(G, x, oc, ou, table, k, kind, param, dup, clip, bank=None, seed=0, offset=0):
    """one launch on poisoned inputs and a guarded NaN xin -> (x after, xin)"""
    b, n = x.shape
    xd = G.poisoned(x.to(DEV))
    xin = G.empty((dup * b, n), dtype=BF16, device=DEV)
    ops.diffusion_sample_step(xd, xin, G.poisoned(oc.to(DEV)), G.poisoned(table.to(DEV)),
                              G.index(torch.tensor([k], dtype=torch.int32, device=DEV)), kind=kind, parameterization=param,
                              out_u=None if ou is None else G.poisoned(ou.to(DEV)), scale=GUIDANCE if ou is not None else 1.0,
                              noise=None if bank is None else G.poisoned(bank.to(DEV)), temperature=TEMPERATURE, clip_last=clip,
                              seed=seed, offset=offset)
    return xd, xin


@pytest.mark.parametrize("kind,param", STEP_FORMS)
@pytest.mark.parametrize("b,n", STEP_SHAPES)
def test_step_kernel_per_element_at_its_edges(G, b, n, kind, param):
    """x after one step == the f32 CPU replica (`torch.equal`: sample.hip keeps the reference's roundings, no contraction,
    IEEE division), and within 1 f32 ulp + 8 units of 2^-24 on cond of the same formulas in float64 (the longest dependent
    chain, DDIM eps, is six f32 roundings; guidance adds two).  With and without guidance (scale 3), xin holding one and
    two copies, clip_last on and off, temperature 0.7, an explicit noise bank, a synthetic 3-row table, k = 0 and k = 2 (the
    last step: the clamp, with values beyond +-1 present).  xin == x.bfloat16() in every copy; k out of range leaves x
    and xin as they were, bit for bit."""
    table = _step_table()
    small = b * n < 100000
    combos = [(g_, dup, clip, k) for g_ in (False, True) for dup in (1, 2) for clip in (False, True) for k in (0, 2)]
    if not small:
        combos = [(True, 2, True, 2), (False, 1, False, 0)]
    for guided, dup, clip, k in combos:
        x, oc, ou, bank = _step_inputs(b, n, guided)
        tag = f"{kind}/{param} B={b} n={n} guided={guided} dup={dup} clip={clip} k={k}"
        clamp = clip and k == 2
        want, _ = _step_replica(x, oc, ou, table[k], bank[k], kind, param, clamp, F32)
        assert want.dtype == F32
        if clamp and b * n >= 1028:
            raw, _ = _step_replica(x, oc, ou, table[k], bank[k], kind, param, False, F32)
            assert bool((raw > 1).any()) and bool((raw < -1).any()), tag
        xd, xin = _run_step(G, x, oc, ou, table, k, kind, param, dup, clip, bank=bank)
        got = xd.cpu()
        bad = got != want
        assert not bool(bad.any()), (tag, int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())
        want64, cond = _step_replica(x, oc, ou, table[k], bank[k], kind, param, clamp, torch.float64)
        assert_elementwise(got, want64, out_dtype=F32, ulps=1, cond=cond, k=8, what=tag)
        for c in range(dup):
            assert torch.equal(xin[c * b:(c + 1) * b].cpu(), got.bfloat16()), (tag, c)
        G.check()
    # k outside the table: nothing is written
    x, oc, ou, bank = _step_inputs(b, n, True)
    for k in (-1, 3):
        xd, xin = _run_step(G, x, oc, ou, table, k, kind, param, 2, True, bank=bank)
        assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32)), (kind, param, k)
        fill = torch.full(tuple(xin.shape), float("nan"), dtype=BF16)  # the guarded allocation's fill, untouched
        assert torch.equal(xin.cpu().view(torch.int16), fill.view(torch.int16)), (kind, param, k)
        G.check()


@pytest.mark.parametrize("kind,param", STEP_FORMS)
def test_step_kernel_with_philox_noise_is_the_replica_on_randn(G, kind, param):
    """without a bank the noise of step k is `ops.randn(total, seed, offset + k * total // 4)` (pinned to the host stream by
    test_gpu_philox.py): x equals the replica fed those normals"""
    table = _step_table()
    seed = 0x123456789ABCDEF0
    for (b, n), offset in (((3, 4), 7), ((1, 1028), 2 ** 32 - 2)):
        total = b * n
        for k in (0, 2):
            x, oc, ou, _ = _step_inputs(b, n, True)
            xi = ops.randn(total, seed, offset + k * total // 4, DEV).cpu().view(b, n)
            want, _ = _step_replica(x, oc, ou, table[k], xi, kind, param, k == 2, F32)
            xd, xin = _run_step(G, x, oc, ou, table, k, kind, param, 1, True, seed=seed, offset=offset)
            assert torch.equal(xd.cpu(), want), (kind, param, b, n, k)
            assert torch.equal(xin.cpu(), want.bfloat16())
    G.check()


@pytest.mark.parametrize("gb", [1, 3])
def test_sample_advance_writes_only_its_entries(G, gb):
    """k += 1 and the gb entries of a guarded timesteps buffer = the next row's t; from the last step the counter becomes
    `steps` and the timesteps stay as they are"""
    table = _step_table()
    td = G.poisoned(table.to(DEV))
    k = G.index(torch.zeros((1,), dtype=torch.int32, device=DEV))
    ts = G.index(torch.full((gb,), -1, dtype=torch.int64, device=DEV))
    for step in range(3):
        ops.diffusion_sample_advance(k, td, ts)
        assert k.item() == step + 1
        assert ts.cpu().tolist() == [int(table[min(step + 1, 2), 0].item())] * gb
    assert k.item() == 3 and ts.cpu().tolist() == [100] * gb
    # from k = steps - 1 with untouched timesteps
    k2 = G.index(torch.full((1,), 2, dtype=torch.int32, device=DEV))
    ts2 = G.index(torch.full((gb,), -7, dtype=torch.int64, device=DEV))
    ops.diffusion_sample_advance(k2, td, ts2)
    assert k2.item() == 3 and ts2.cpu().tolist() == [-7] * gb
    G.check()
