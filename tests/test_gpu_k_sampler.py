"""The sigma-space samplers k_euler_a / k_heun / k_dpmpp_2m on the GPU (csrc/sample.hip: sample_step_kernel, diffusion.
make_sampler) against the reference's own (tests/golden/k_samplers.pt, tools/gen_k_sampler_golden.py): the float timestep
embedding, the fused step kernel teacher-forced and free-running on the recorded model outputs and draws, per element at its
edges against an f32 CPU replica and float64, its Philox draws, end-to-end sampling with the small UNet against the reference's
fp32 run with its bf16-autocast distance as the yardstick, the timesteps the UNet is handed, graph == eager, the first stage."""
import math

import pytest
import torch

import cflearn_amd as C
from cflearn_amd import ops
from cflearn_amd.diffusion import NoiseSchedule, k_sampler_table, make_sampler
from helpers import assert_elementwise, guarded_ops
from k_sampler_replay import COL, decode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
KINDS = ("k_euler_a", "k_heun", "k_dpmpp_2m")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("k_samplers.pt")


@pytest.fixture(scope="module")
def decoded(fx):
    """every step record decoded once (the numpy-f32 replay of the host test, each image checked against the reference's hash)"""
    return [(r, decode(fx, r)) for r in fx["steps"]]


@pytest.fixture(scope="module")
def small(golden):
    u = golden("unet_small.pt")
    m = C.build_module("unet_diffuser", config=dict(u["cfg"]))
    m.load_state_dict(u["sd"])
    return m.to(DEV)


@pytest.fixture
def G(monkeypatch):
    g = guarded_ops(monkeypatch)
    yield g
    g.check()


# ---------------------------------------------------------------------------------------------
# the float timestep embedding
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dim", [320, 321])
def test_float_timestep_embedding(G, dim):
    """float t against the float64 formula with the int test's tolerance (test_gpu_unet.py: 5e-4 for arguments up to 999), and
    per element with the int edge test's error model; integral float t is the int64 entry bit for bit"""
    t = torch.tensor([0.0, 0.5, 142.7142791748047, 999.0])
    out = ops.timestep_embedding(G.poisoned(t.to(DEV)), dim)
    assert tuple(out.shape) == (4, dim) and out.dtype == F32
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    arg = t.double()[:, None] * freqs[None]
    want = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    cond = torch.cat([arg, arg], 1)
    if dim % 2:
        want = torch.cat([want, torch.zeros(len(t), 1, dtype=torch.float64)], 1)
        cond = torch.cat([cond, torch.zeros(len(t), 1, dtype=torch.float64)], 1)
        assert bool((out[:, -1] == 0).all())
    err = (out.cpu().double() - want).abs().max().item()
    print(f"float timestep embedding dim {dim}: max abs error {err:.3e}")
    assert err < 5e-4
    # (the argument's ~3 roundings in the exponent put it off by up to ~32 units of 2^-24 of itself: test_gpu_kernel_edges.py)
    assert_elementwise(out, want, out_dtype=F32, ulps=4, cond=cond, k=32, what=f"float timestep embedding dim {dim}")
    ti = torch.tensor([0, 1, 37, 500, 999])
    assert torch.equal(ops.timestep_embedding(G.poisoned(ti.float().to(DEV)), dim), ops.timestep_embedding(G.index(ti.to(DEV)), dim))
    G.check()


# ---------------------------------------------------------------------------------------------
# the step kernel on the reference's records
# ---------------------------------------------------------------------------------------------


def _outs(r, d, e):
    b = d["states"].shape[1]
    o = d["outputs"][e].to(DEV).bfloat16()
    assert torch.equal(o.float().cpu(), d["outputs"][e])  # the recorded outputs are bf16 values
    return (o, None) if r["scale"] is None else (o[:b].contiguous(), o[b:].contiguous())


def _aux(r, t):
    return None if r["kind"] == "k_euler_a" else t.to(DEV).contiguous().clone()


def test_step_kernel_teacher_forced_is_the_replay_bit_for_bit(decoded):
    """every recorded evaluation of every record: the reference's state (and the carried d / old_denoised), model output(s),
    draw and scalars in; x and aux out equal the numpy-f32 replay (whose images carry the reference's hashes) bit for bit, and
    xin = bf16(next input * c_in) in both copies"""
    assert len(decoded) == 12
    for r, d in decoded:
        table = d["table"].to(DEV)
        bank = None if d["noises"] is None else d["noises"].to(DEV).contiguous()
        b = d["states"].shape[1]
        for e in range(table.shape[0]):
            x = d["states"][e].to(DEV).contiguous().clone()
            aux = _aux(r, d["auxs"][e])
            xin = torch.empty((2 * b,) + tuple(x.shape[1:]), dtype=BF16, device=DEV)
            oc, ou = _outs(r, d, e)
            ops.k_sample_step(x, aux, xin, oc, table, torch.tensor([e], dtype=torch.int32, device=DEV), kind=r["kind"],
                              parameterization=r["parameterization"], out_u=ou, scale=r["scale"] or 1.0, noise=bank)
            tag = (r["kind"], r["parameterization"], r["scale"], e)
            assert torch.equal(x.cpu(), d["states"][e + 1]), tag
            if aux is not None:
                assert torch.equal(aux.cpu(), d["auxs"][e + 1]), tag
            want_in = (d["nexts"][e] * d["table"][e, COL["c_in_next"]]).bfloat16()
            assert torch.equal(xin[:b].cpu(), want_in) and torch.equal(xin[b:].cpu(), want_in), tag


def test_step_kernel_free_run_on_the_recorded_outputs(decoded):
    """all evaluations chained on the device from z * sigmas[0] (advance bumps k and writes the next timestep, f32 or int64):
    the counter ends at the number of evaluations, the timesteps buffer holds the table's next entry after each advance, and
    the image after every reference step is within 1e-5 relative L2 (the DDIM free-run bound of test_gpu_sampler.py)"""
    for r, d in decoded:
        table = d["table"].to(DEV)
        bank = None if d["noises"] is None else d["noises"].to(DEV).contiguous()
        evals, per = table.shape[0], 2 if r["kind"] == "k_heun" else 1
        x = d["states"][0].to(DEV).contiguous().clone()
        aux = _aux(r, d["auxs"][0])
        xin = torch.empty_like(x, dtype=BF16)
        k = torch.zeros((1,), dtype=torch.int32, device=DEV)
        ts = torch.full((x.shape[0],), -1, dtype=torch.int64 if r["quantize"] else F32, device=DEV)
        worst = 0.0
        for e in range(evals):
            oc, ou = _outs(r, d, e)
            ops.k_sample_step(x, aux, xin, oc, table, k, kind=r["kind"], parameterization=r["parameterization"], out_u=ou,
                              scale=r["scale"] or 1.0, noise=bank)
            ops.k_sample_advance(k, table, ts)
            if e + 1 < evals:
                assert ts.dtype == r["timesteps"].dtype and torch.equal(ts.cpu(), r["timesteps"][e + 1].expand(x.shape[0])), (r["kind"], e)
            if (e + 1) % per == 0:
                want = d["images"][(e + 1) // per]
                worst = max(worst, ((x.cpu() - want).norm() / want.norm()).item())
        assert k.item() == evals
        assert worst <= 1e-5, (r["kind"], r["parameterization"], r["scale"], worst)


# ---------------------------------------------------------------------------------------------
# the step kernel per element at its edges: an f32 CPU replica (bit-equal) and the same formulas in float64
# ---------------------------------------------------------------------------------------------

STEP_GROUPS = 2048 * 256  # groups of 4 elements one pass of sample_step_kernel's stride loop covers
STEP_SHAPES = [(1, 4), (3, 4), (1, 1028), (2, 4 * (STEP_GROUPS // 2 + 2))]  # the last: 524 292 groups, a second pass
GUIDANCE = 3.0
# row flags of the synthetic 3-row table: euler_a with the draw, without it, with it (last row: the clamp); heun stage 1,
# stage 2, stage 2 (last); dpmpp_2m first evaluation, later, later (last)
FLAGS = {"k_euler_a": (1.0, 0.0, 1.0), "k_heun": (0.0, 1.0, 1.0), "k_dpmpp_2m": (0.0, 1.0, 1.0)}
# f32 roundings on the longest dependent chain to the state (sample_step_kernel's order), without guidance:
#   euler_a      m c_out | img - . | img - den | / sigma | d dt | img + . | + xi sigma_up                      7
#   heun stage 1 the same up to d (4: aux), then d dt | x + . (the next input)                                 6
#   heun stage 2 aux dt | x + . (img) | img - m c_out | img - den | / sigma | aux + d | / 2 | . dt | x + .     9
#   dpmpp_2m     m c_out | img - . (den: aux) | r_plus den | - r_minus aux | expm1 . | ratio img - .           6  (first: 4)
# the guidance mix m = u + s (m - u) sits in front of m c_out: 3 more; xin = bf16(next input * c_in): 1 more, rounded to bf16
CHAIN = {"k_euler_a": 7, "k_heun": 9, "k_dpmpp_2m": 6}


def _k_table(kind):
    """3 rows: a timestep and coefficients in [0.2, 1.5] (dt negative, as sigmas fall), the flags of FLAGS"""
    t = torch.rand((3, ops.KSAMPLE_ROW), generator=torch.Generator().manual_seed(13)) * 1.3 + 0.2
    t[:, COL["t"]] = torch.tensor([900.5, 500.25, 100.0])
    t[:, COL["dt"]] = -t[:, COL["dt"]]
    t[:, COL["flag"]] = torch.tensor(FLAGS[kind])
    return t


def _k_replica(kind, par, row, x, aux, oc, ou, xi, clamp, dtype):
    """sample_step_kernel's documented operation order with torch CPU ops in `dtype`, one rounding per operation and no FMA
    (every line is one torch op on materialised operands) -> ({x, aux, next, xin}, the same formulas on absolute values).
    `aux` / `x` come back as they were where the kernel does not write them."""
    c = {n: row[i].to(dtype) for n, i in COL.items()}
    ca = {n: v.abs() for n, v in c.items()}  # (the real tables hold negative dt and expm1(-h))
    flag = bool(row[COL["flag"]] != 0)
    scale = torch.tensor(GUIDANCE, dtype=F32).to(dtype)
    x, m = x.to(dtype), oc.to(dtype)
    am = m.abs()
    if ou is not None:  # u + scale * (m - u)
        u = ou.to(dtype)
        t = m - u
        t = scale * t
        m = u + t
        am = u.abs() + scale.abs() * (am + u.abs())
    a_in = None if aux is None else aux.to(dtype)
    img, aimg = x, x.abs()
    if kind == "k_heun" and flag:
        t = a_in * c["dt"]
        img = x + t
        aimg = x.abs() + a_in.abs() * ca["dt"]
    t = m * c["c_out"]
    if par == "v":
        s = img * c["c_skip"]
        den = s - t
        aden = aimg * ca["c_skip"] + am * ca["c_out"]
    else:
        den = img - t
        aden = aimg + am * ca["c_out"]
    a_out, a_aux = a_in, None if a_in is None else a_in.abs()
    if kind == "k_dpmpp_2m":
        dd, add = den, aden
        if flag:
            p = c["r_plus"] * den
            q = c["r_minus"] * a_in
            dd = p - q
            add = ca["r_plus"] * aden + ca["r_minus"] * a_in.abs()
        p = c["sigma_ratio"] * img
        q = c["expm1_neg_h"] * dd
        y = p - q
        ay = ca["sigma_ratio"] * aimg + ca["expm1_neg_h"] * add
        a_out, a_aux, nxt, anxt = den, aden, y, ay
    else:
        t = img - den
        d = t / c["sigma"]
        ad = (aimg + aden) / ca["sigma"]
        if kind == "k_euler_a":
            t = d * c["dt"]
            y = img + t
            ay = aimg + ad * ca["dt"]
            if flag:
                t = xi.to(dtype) * c["sigma_up"]
                y = y + t
                ay = ay + xi.to(dtype).abs() * ca["sigma_up"]
            nxt, anxt = y, ay
        elif not flag:  # heun stage 1
            t = d * c["dt"]
            nxt = x + t
            anxt = x.abs() + ad * ca["dt"]
            y, ay, a_out, a_aux = x, x.abs(), d, ad
        else:  # heun stage 2
            t = a_in + d
            t = t / torch.tensor(2.0, dtype=dtype)
            t = t * c["dt"]
            y = x + t
            ay = x.abs() + (a_in.abs() + ad) / 2 * ca["dt"]
            nxt, anxt = y, ay
    if clamp and not (kind == "k_heun" and not flag):
        y = y.clamp(-1.0, 1.0)
        nxt = y
    return (dict(x=y, aux=a_out, next=nxt, xin=nxt * c["c_in_next"]),
            dict(x=ay, aux=a_aux, next=anxt, xin=anxt * ca["c_in_next"]))


def _k_inputs(b, n, guided, kind):
    g = torch.Generator().manual_seed(1000 * b + n)
    x = torch.randn((b, n), generator=g) * 1.5
    oc = torch.randn((b, n), generator=g).to(BF16)
    ou = torch.randn((b, n), generator=g).to(BF16) if guided else None
    bank = torch.randn((3, b, n), generator=g) if kind == "k_euler_a" else None
    aux = None if kind == "k_euler_a" else torch.randn((b, n), generator=g)
    return x, aux, oc, ou, bank


def _run_k(G, x, aux, oc, ou, table, k, kind, par, dup, clip, bank=None, seed=0, offset=0):
    """one launch on poisoned inputs and a guarded NaN xin -> (x after, aux after, xin)"""
    b, n = x.shape
    xd = G.poisoned(x.to(DEV))
    ad = None if aux is None else G.poisoned(aux.to(DEV))
    xin = G.empty((dup * b, n), dtype=BF16, device=DEV)
    ops.k_sample_step(xd, ad, xin, G.poisoned(oc.to(DEV)), G.poisoned(table.to(DEV)),
                      G.index(torch.tensor([k], dtype=torch.int32, device=DEV)), kind=kind, parameterization=par,
                      out_u=None if ou is None else G.poisoned(ou.to(DEV)), scale=GUIDANCE if ou is not None else 1.0,
                      noise=None if bank is None else G.poisoned(bank.to(DEV)), clip_last=clip, seed=seed, offset=offset)
    return xd, ad, xin


@pytest.mark.parametrize("par", ["eps", "v"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,n", STEP_SHAPES)
def test_k_step_kernel_per_element_at_its_edges(G, b, n, kind, par):
    """x, aux and xin after one launch == the f32 CPU replica (`torch.equal`: the kernel keeps the reference's roundings, no
    contraction, IEEE division), and within 1 ulp + k units of 2^-24 on cond of the same formulas in float64, cond = the formula
    on absolute values ((x - denoised) / sigma cancels: the error scales with |x|, not with the result) and k = the f32
    roundings on the longest dependent chain of the kind (CHAIN above: euler_a 7, heun 9, dpmpp_2m 6), + 3 under guidance, + 1
    for xin.  Rows 0, 1, 2 of a synthetic table: first evaluation / stage 1 / no history, the other flag value, and the last
    row (the clamp, with values beyond +-1 present); with and without guidance (scale 3), xin in one and two copies, clip_last
    on and off, an explicit bank for euler_a.  An aux the row does not read (heun stage 1, dpmpp_2m's first evaluation) is NaN
    on entry.  k = -1 and k = rows leave x, aux and xin as they were, bit for bit."""
    table = _k_table(kind)
    small = b * n < 100000
    combos = [(g_, dup, clip, k) for g_ in (False, True) for dup in (1, 2) for clip in (False, True) for k in (0, 1, 2)]
    if not small:
        combos = [(True, 2, True, 2), (False, 1, False, 0)]
    for guided, dup, clip, k in combos:
        x, aux, oc, ou, bank = _k_inputs(b, n, guided, kind)
        tag = f"{kind}/{par} B={b} n={n} guided={guided} dup={dup} clip={clip} k={k}"
        reads_aux = kind != "k_euler_a" and FLAGS[kind][k] != 0
        if aux is not None and not reads_aux:
            aux = torch.full_like(aux, float("nan"))
        clamp = clip and k == 2
        xi = None if bank is None else bank[k]
        want, _ = _k_replica(kind, par, table[k], x, aux, oc, ou, xi, clamp, F32)
        assert want["x"].dtype == F32 and bool(torch.isfinite(want["x"]).all())
        if clamp and b * n >= 1028:
            raw, _ = _k_replica(kind, par, table[k], x, aux, oc, ou, xi, False, F32)
            assert bool((raw["x"] > 1).any()) and bool((raw["x"] < -1).any()), tag
        xd, ad, xin = _run_k(G, x, aux, oc, ou, table, k, kind, par, dup, clip, bank=bank)
        got = xd.cpu()
        bad = got != want["x"]
        assert not bool(bad.any()), (tag, int(bad.sum()), got[bad][:4].tolist(), want["x"][bad][:4].tolist())
        kk = CHAIN[kind] + (3 if guided else 0)
        want64, cond = _k_replica(kind, par, table[k], x, aux, oc, ou, xi, clamp, torch.float64)
        assert_elementwise(got, want64["x"], out_dtype=F32, ulps=1, cond=cond["x"], k=kk, what=tag + " x")
        if ad is not None:
            if reads_aux and kind == "k_heun":  # stage 2 leaves the saved d
                assert torch.equal(ad.cpu(), aux), tag
            else:
                assert torch.equal(ad.cpu(), want["aux"]), tag
                assert_elementwise(ad.cpu(), want64["aux"], out_dtype=F32, ulps=1, cond=cond["aux"], k=kk, what=tag + " aux")
        for c in range(dup):
            assert torch.equal(xin[c * b:(c + 1) * b].cpu(), want["xin"].bfloat16()), (tag, c)
        assert_elementwise(xin[:b], want64["xin"], out_dtype=BF16, ulps=1, cond=cond["xin"], k=kk + 1, what=tag + " xin")
        G.check()
    # k outside the table: nothing is written
    x, aux, oc, ou, bank = _k_inputs(b, n, True, kind)
    for k in (-1, 3):
        xd, ad, xin = _run_k(G, x, aux, oc, ou, table, k, kind, par, 2, True, bank=bank)
        assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32)), (kind, par, k)
        if ad is not None:
            assert torch.equal(ad.cpu().view(torch.int32), aux.view(torch.int32)), (kind, par, k)
        fill = torch.full(tuple(xin.shape), float("nan"), dtype=BF16)  # the guarded allocation's fill, untouched
        assert torch.equal(xin.cpu().view(torch.int16), fill.view(torch.int16)), (kind, par, k)
        G.check()


@pytest.mark.parametrize("par", ["eps", "v"])
def test_k_euler_a_with_philox_noise_is_the_replica_on_randn(G, par):
    """without a bank the draw of evaluation k is `ops.randn(total, seed, offset + k * total // 4)` (pinned to the host stream by
    test_gpu_philox.py): x equals the replica fed those normals"""
    table = _k_table("k_euler_a")
    seed = 0x123456789ABCDEF0
    for (b, n), offset in (((3, 4), 7), ((1, 1028), 2 ** 32 - 2)):
        total = b * n
        for k in (0, 2):
            x, aux, oc, ou, _ = _k_inputs(b, n, True, "k_euler_a")
            xi = ops.randn(total, seed, offset + k * total // 4, DEV).cpu().view(b, n)
            want, _ = _k_replica("k_euler_a", par, table[k], x, None, oc, ou, xi, k == 2, F32)
            xd, _, xin = _run_k(G, x, None, oc, ou, table, k, "k_euler_a", par, 1, True, seed=seed, offset=offset)
            assert torch.equal(xd.cpu(), want["x"]), (par, b, n, k)
            assert torch.equal(xin.cpu(), want["xin"].bfloat16())
    G.check()


@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("gb", [1, 3])
def test_k_advance_writes_only_its_entries(G, gb, quantize):
    """k += 1 and the gb entries of a guarded timesteps buffer = the next row's t (f32 as it stands, or its int64); from the
    last row the counter becomes `rows` and the timesteps stay"""
    table = _k_table("k_heun")
    td = G.poisoned(table.to(DEV))
    dt = torch.int64 if quantize else F32
    cast = (lambda v: int(v)) if quantize else float
    k = G.index(torch.zeros((1,), dtype=torch.int32, device=DEV))
    ts = torch.full((gb,), -1, dtype=dt, device=DEV)
    ts = G.index(ts) if quantize else G.poisoned(ts)
    for step in range(3):
        ops.k_sample_advance(k, td, ts)
        assert k.item() == step + 1
        assert ts.cpu().tolist() == [cast(table[min(step + 1, 2), 0].item())] * gb
    assert k.item() == 3 and ts.cpu().tolist() == [cast(100.0)] * gb
    assert table[1, 0].item() == 500.25  # a fractional timestep went through as it is (or truncated to its index)
    G.check()


# ---------------------------------------------------------------------------------------------
# end to end around the small UNet
# ---------------------------------------------------------------------------------------------


def _per_sample(a, ref):
    a, ref = a.float().cpu().flatten(1), ref.float().flatten(1)
    return ((a - ref).norm(dim=1) / ref.norm(dim=1)).tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_k_end_to_end_small_unet_within_the_reference_bf16_distance(fx, small, kind):
    """Per-sample relative L2 against the reference's fp32 run <= 1.1 x the reference's own bf16-autocast distance (the margin
    test_gpu_sampler.py holds DDIM and basic to); 12 steps, guidance 3.0, float timesteps, recorded noise for k_euler_a."""
    e = fx["e2e"]
    s = make_sampler(kind, small, NoiseSchedule(device=DEV), unconditional_cond=e["uncond"], unconditional_guidance_scale=e["scale"])
    kw = dict(cond=e["cond"].to(DEV), num_steps=e["steps"])
    if kind == "k_euler_a":
        kw["noise"] = e["k_euler_a_noise_q"].float() * e["k_euler_a_noise_scale"]
    y = s.sample(e["z"].to(DEV), clip_output=False, **kw)
    mine, yard = _per_sample(y, e[f"{kind}_fp32"]), _per_sample(e[f"{kind}_autocast"], e[f"{kind}_fp32"])
    print(f"{kind} e2e per-sample rel-L2 vs fp32: HIP {mine}, reference bf16 autocast {yard}, "
          f"ratio {[a / b for a, b in zip(mine, yard)]}")
    for a, b in zip(mine, yard):
        assert a <= 1.1 * b, (mine, yard)
    yc = s.sample(e["z"].to(DEV), **kw)  # clip_output=True: the last evaluation clamps
    assert torch.equal(yc, y.clamp(-1.0, 1.0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("quantize", [False, True])
def test_timesteps_handed_to_the_unet(fx, small, kind, quantize):
    """`default_quantize=True` hands the UNet int64 timesteps equal to the fixture's, False the fractional f32 ones (one per
    sigma; k_heun's second stage evaluates at the next sigma's); num_steps = 1 evaluates nothing and returns z * sigmas[0]"""
    rec = next(t for t in fx["tables"] if t["sigmas_scheduler"] is None and t["quantize"] == quantize and t["steps"] == 8)
    seen = []
    hook = small.register_forward_pre_hook(lambda mod, args, kwargs: seen.append(kwargs["timesteps"].clone()), with_kwargs=True)
    try:
        s = make_sampler(kind, small, NoiseSchedule(device=DEV), default_quantize=quantize)
        y = s.sample(num_samples=2, shape=(3, 16, 16), cond=fx["e2e"]["cond"].to(DEV), num_steps=8, seed=3)
        n_seen = len(seen)
        z = torch.randn((2, 3, 16, 16), generator=torch.Generator().manual_seed(4)).to(DEV)
        one = s.sample(z, num_steps=1, clip_output=False)
        one_clipped = s.sample(z, num_steps=1)
    finally:
        hook.remove()
    assert torch.isfinite(y).all() and len(seen) == n_seen  # (num_steps = 1: no forward)
    idx = list(range(7)) if kind != "k_heun" else [i for st in range(7) for i in (st, st + 1)]
    want = rec["timesteps"][idx]
    assert len(seen) == len(idx)
    got = torch.stack([t.cpu() for t in seen])
    assert got.dtype == (torch.int64 if quantize else F32) and bool((got == got[:, :1]).all())
    if quantize:
        assert torch.equal(got[:, 0], want)
    else:
        assert bool((want.frac() != 0).any())
        ulp = torch.ldexp(torch.ones_like(want), (torch.frexp(want.abs().clamp_min(2.0 ** -126))[1] - 24).to(torch.int32))
        assert bool(((got[:, 0] - want).abs() <= ulp).all()), (got[:, 0], want)  # (1 ulp: the host's log, test_k_sampler_host.py)
    sigma0 = k_sampler_table("k_euler_a", NoiseSchedule(), 2)[0, COL["sigma"]]
    assert torch.equal(one.cpu(), z.cpu() * sigma0) and torch.equal(one_clipped, one.clamp(-1.0, 1.0))


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("kind", ["k_heun", "k_euler_a"])
def test_k_graph_equals_eager_bit_for_bit(fx, small, kind, guided):
    """the recorded unit is one evaluation (k_heun: two per step); k_euler_a draws from Philox inside the recorded launch"""
    e = fx["e2e"]
    cfg = {} if not guided else dict(unconditional_cond=e["uncond"], unconditional_guidance_scale=3.0)
    s = make_sampler(kind, small, NoiseSchedule(device=DEV), **cfg)
    kw = dict(num_samples=2, shape=(3, 16, 16), cond=e["cond"].to(DEV), num_steps=6, seed=5)
    eager = s.sample(**kw)
    graph = s.sample(**kw, use_graph=True)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph), (eager - graph).abs().max().item()
    assert not torch.equal(s.sample(**dict(kw, seed=6)), eager)


@pytest.mark.parametrize("kind", KINDS)
def test_k_latent_sampler_decodes(kind):
    """with a first stage the default returns its decode of latent / scale, `return_latent=True` the latent itself"""
    from test_gpu_first_stage import SCALE, _small_ae, _small_unet

    ae, _ = _small_ae()
    unet = _small_unet().eval()
    z = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(23)).to(DEV)
    sampler = make_sampler(kind, unet, NoiseSchedule(device=DEV), first_stage=ae, first_stage_scale_factor=SCALE)
    img = sampler.sample(z, num_steps=3, seed=9)
    latent = sampler.sample(z, num_steps=3, seed=9, return_latent=True)
    assert tuple(latent.shape) == (2, 4, 8, 8) and latent.dtype == F32 and tuple(img.shape) == (2, 3, 16, 16)
    with torch.no_grad():
        want = ae.decode(C.DecoderInputs(z=latent / SCALE))
    assert torch.equal(img, want)
    assert float(latent.abs().max()) <= 1.0  # clip_output acts on the latent
    plain = make_sampler(kind, unet, NoiseSchedule(device=DEV)).sample(z, num_steps=3, seed=9)
    assert torch.equal(plain, latent)
