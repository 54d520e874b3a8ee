"""The sigma-space samplers (k_euler_a, k_heun, k_dpmpp_2m), host side (no GPU): the sigma / timestep tables and the
per-evaluation step table against the reference's (tests/golden/k_samplers.pt, tools/gen_k_sampler_golden.py), the kernel's
documented operation order in numpy f32 reproducing every recorded image, the refusals, and the C-ABI rows."""
import os
import re

import pytest
import torch

import cflearn_amd  # noqa: F401
from cflearn_amd import _lib, ops
from cflearn_amd.diffusion import (K_COLUMNS, KDiffusionSampler, NoiseSchedule, get_ancestral_step, k_sampler_table, k_sigma_tables,
                                   make_sampler)
from k_sampler_replay import COL, decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("k_euler_a", "k_heun", "k_dpmpp_2m")
# Columns whose values pass through log / exp / pow / expm1, which a host's math library need not round correctly: 1 f32 ulp.
# `sigma` and everything formed from it: the default schedule is exp() of interpolated log sigmas, karras a pow; dt, sigma_up,
# c_out, c_skip, c_in_next, sigma_ratio are correctly rounded operations ON such a sigma, so they inherit its one ulp only when
# it differs, which the test of `sigma` itself then reports; they are compared bit for bit given equal sigmas.
# `t` (float form) interpolates log sigma; expm1_neg_h, r_plus, r_minus go through log and expm1.
ULP_COLUMNS = ("t", "expm1_neg_h", "r_plus", "r_minus")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("k_samplers.pt")


def _eq(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), f"{what}: max diff {(a.double() - b.double()).abs().max().item()}"


def _within_one_ulp(a, b, what):
    """f32 tensors equal up to one unit in the last place of the reference value"""
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    ulp = torch.ldexp(torch.ones_like(b), (torch.frexp(b.abs().clamp_min(2.0 ** -126))[1] - 24).to(torch.int32))
    bad = (a - b).abs() > ulp
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} entries beyond 1 ulp, e.g. {a[bad][:3].tolist()} vs {b[bad][:3].tolist()}"


def test_sigma_and_timestep_tables_equal_the_reference(fx):
    """`sigmas_base` is correctly rounded arithmetic on the f32 alphas: bit for bit.  `log_sigmas_base` (log), `sigmas` (exp of
    the interpolated logs / karras' pow) and the float timesteps (interpolated in log sigma) may differ by 1 f32 ulp; the
    quantised timesteps are indices: equal."""
    assert len(fx["tables"]) == 8
    seen = set()
    for rec in fx["tables"]:
        tb = k_sigma_tables(NoiseSchedule(), rec["steps"], rec["sigmas_scheduler"], rec["quantize"])
        what = f"{rec['sigmas_scheduler']}/quantize {rec['quantize']}/{rec['steps']}"
        seen.add((rec["sigmas_scheduler"], rec["quantize"], rec["steps"]))
        _eq(tb["sigmas_base"], fx["sigmas_base"], "sigmas_base")
        _within_one_ulp(tb["log_sigmas_base"], fx["log_sigmas_base"], "log_sigmas_base")
        assert tb["sigmas"].shape == (rec["steps"] + 1,) and tb["sigmas"][-1].item() == 0.0
        _within_one_ulp(tb["sigmas"], rec["sigmas"], f"{what} sigmas")
        if rec["quantize"]:
            _eq(tb["timesteps"], rec["timesteps"], f"{what} timesteps")
            assert tb["timesteps"].dtype == torch.int64
        else:
            _within_one_ulp(tb["timesteps"], rec["timesteps"], f"{what} timesteps")
            assert bool((tb["timesteps"].frac() != 0).any()), "the float timesteps are fractional"
    assert seen == {(s, q, n) for s in (None, "karras") for q in (False, True) for n in (8, 25)}
    # the run ends at sigma_min: the last sigma a step reaches is the schedule's first
    tb = k_sigma_tables(NoiseSchedule(), 8)
    # (exp(log(sigma_min)): the rounding of the log, |log| ~ 3.5, is magnified by that much: a few ulps, far inside 1e-6)
    assert abs(tb["sigmas"][7].item() / tb["sigmas_base"][0].item() - 1.0) < 1e-6
    assert tb["timesteps"][0].item() == 999.0 and tb["timesteps"][7].item() == 0.0


def test_step_table_equals_the_reference_scalars(fx):
    assert len(fx["steps"]) == 12 and tuple(fx["columns"]) == K_COLUMNS == tuple(COL)
    for r in fx["steps"]:
        s = NoiseSchedule(parameterization=r["parameterization"])
        tb = k_sampler_table(r["kind"], s, r["steps"], sigmas_scheduler=r["sigmas_scheduler"], quantize=r["quantize"])
        evals = (r["steps"] - 1) * (2 if r["kind"] == "k_heun" else 1)
        assert tb.shape == (evals, ops.KSAMPLE_ROW) == tuple(r["table"].shape)
        what = f"{r['kind']} {r['parameterization']} {r['sigmas_scheduler']}"
        _within_one_ulp(tb[:, COL["sigma"]], r["table"][:, COL["sigma"]], f"{what} sigma")
        same_sigma = torch.equal(tb[:, COL["sigma"]], r["table"][:, COL["sigma"]])
        for name, i in COL.items():
            if name in ULP_COLUMNS and not (name == "t" and r["quantize"]):
                _within_one_ulp(tb[:, i], r["table"][:, i], f"{what} {name}")
            elif name != "sigma" and same_sigma:
                _eq(tb[:, i], r["table"][:, i], f"{what} {name}")
        if r["quantize"]:
            assert torch.equal(tb[:, 0], r["timesteps"].float()) and r["timesteps"].dtype == torch.int64
        else:
            assert r["timesteps"].dtype == torch.float32


def test_kernel_order_in_numpy_reproduces_every_reference_image(fx):
    """z * sigmas[0], then the documented per-evaluation arithmetic on the recorded outputs, draws and scalars: the SHA-256 of
    the image after every reference step (decode asserts each), the last step returning the image as it is"""
    for r in fx["steps"]:
        d = decode(fx, r)
        assert d["images"].shape == (r["steps"] + 1, *fx["step_z"].shape)
        assert torch.equal(d["images"][-1], d["images"][-2])
        if r["kind"] == "k_heun":  # stage 1 leaves the state, stage 2 the saved d
            assert torch.equal(d["states"][1], d["states"][0]) and torch.equal(d["auxs"][2], d["auxs"][1])


def test_table_structure_per_kind():
    s = NoiseSchedule()
    e = k_sampler_table("k_euler_a", s, 6)
    assert e.shape == (5, ops.KSAMPLE_ROW) and bool((e[:, COL["flag"]] == 1).all()) and bool((e[:, COL["sigma_up"]] > 0).all())
    h = k_sampler_table("k_heun", s, 6)
    assert h.shape == (10, ops.KSAMPLE_ROW) and h[:, COL["flag"]].tolist() == [0.0, 1.0] * 5
    assert torch.equal(h[0::2, COL["dt"]], h[1::2, COL["dt"]])
    assert torch.equal(h[1:-1:2, COL["sigma"]], h[2::2, COL["sigma"]])  # stage 2 evaluates at the next step's sigma
    assert torch.equal(h[0::2, COL["c_in_next"]], h[1::2, COL["c_in_next"]])
    m = k_sampler_table("k_dpmpp_2m", s, 6)
    assert m.shape == (5, ops.KSAMPLE_ROW) and m[:, COL["flag"]].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0]
    for kind in KINDS:
        assert k_sampler_table(kind, s, 1).shape == (0, ops.KSAMPLE_ROW)
    down, up = get_ancestral_step(2.0, 1.0)
    assert abs(down ** 2 + up ** 2 - 1.0) < 1e-12 and get_ancestral_step(2.0, 1.0, eta=0.0) == (1.0, 0.0)


class _Tiny(torch.nn.Module):
    in_channels = 3

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_refusals_and_config():
    u = _Tiny()
    for kind in KINDS:
        with pytest.raises(ValueError):
            make_sampler(kind, u, NoiseSchedule(parameterization="x0"))
        with pytest.raises(ValueError):
            make_sampler(kind, u, sigmas_scheduler="exponential")
        with pytest.raises(ValueError):
            make_sampler(kind, u, unconditional_cond=torch.zeros(2, 3, 4))
        with pytest.raises(NotImplementedError):
            make_sampler(kind, u, unconditional_cond={"concat": torch.zeros(1, 2, 3)})
        with pytest.raises(TypeError):
            make_sampler(kind, u, eta=0.5)  # a DDIM key
        s = make_sampler(kind, u)
        assert isinstance(s, KDiffusionSampler) and s.default_steps == 25 and not s.default_quantize and s.sigmas_scheduler is None
        for kw in (dict(ref=torch.zeros(1), ref_mask=torch.zeros(1)), dict(start_step=3), dict(step_callback=print)):
            with pytest.raises(NotImplementedError):
                s.sample(torch.zeros(1, 3, 4, 4), **kw)
        with pytest.raises(TypeError):
            s.sample(torch.zeros(1, 3, 4, 4), bogus=1)
        with pytest.raises(RuntimeError):  # the UNet lives on the CPU: no eager fallback
            s.sample(torch.zeros(1, 3, 4, 4))
    s = make_sampler("k_dpmpp_2m", u, default_quantize=True, sigmas_scheduler="karras", default_steps=9,
                     unconditional_cond=torch.zeros(1, 2, 3), unconditional_guidance_scale=7.5)
    assert s.default_quantize and s.sigmas_scheduler == "karras" and s.default_steps == 9 and s.unconditional_guidance_scale == 7.5
    for kind in ("k_euler", "klms", "plms", "solver", "lcm"):
        with pytest.raises(NotImplementedError):
            make_sampler(kind, u)
    with pytest.raises(ValueError):
        k_sampler_table("ddim", NoiseSchedule(), 5)
    with pytest.raises(ValueError):
        k_sigma_tables(NoiseSchedule(), 0)


def test_noise_bank_refusals():
    """the bank is checked before anything touches the device: heun / 2m take none, euler_a's is [num_steps - 1, B, C, H, W]"""
    u = _Tiny()
    z = torch.zeros(2, 3, 4, 4)
    for kind in ("k_heun", "k_dpmpp_2m"):
        with pytest.raises(ValueError, match="draws no noise"):
            make_sampler(kind, u).sample(z, num_steps=5, noise=torch.zeros(4, 2, 3, 4, 4))
    s = make_sampler("k_euler_a", u)
    for shape in ((5, 2, 3, 4, 4), (4, 2, 3, 4, 5), (4, 1, 3, 4, 4)):
        with pytest.raises(ValueError, match="noise bank"):
            s.sample(z, num_steps=5, noise=torch.zeros(shape))
        with pytest.raises(ValueError, match="noise bank"):
            s.sample(num_samples=2, shape=(3, 4, 4), num_steps=5, noise=torch.zeros(shape))
    with pytest.raises(RuntimeError):  # a well-shaped bank passes the check and reaches the device test
        s.sample(z, num_steps=5, noise=torch.zeros(4, 2, 3, 4, 4))


def test_k_sampler_symbols_constants_and_null_arguments():
    text = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    for name in ("cfhip_k_sample_step", "cfhip_k_sample_advance", "cfhip_timestep_embedding_f32"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    assert f"#define CFHIP_KSAMPLE_ROW {ops.KSAMPLE_ROW}" in text and ops.KSAMPLE_ROW == 12 == len(K_COLUMNS)
    assert ops.KSAMPLERS == {"k_euler_a": 0, "k_heun": 1, "k_dpmpp_2m": 2}
    assert ops.SAMPLE_ROW == 8 and ops.SAMPLERS == {"ddim": 0, "basic": 1}  # the DDIM constants stay
    for line in ("k_samplers.py", "CFHIP_KSAMPLER_EULER_A", "CFHIP_KSAMPLER_HEUN", "CFHIP_KSAMPLER_DPMPP_2M"):
        assert line in text
    lib = _lib.load()  # the C-ABI rejects null arguments with -1 before any launch
    assert lib.cfhip_k_sample_step(None, None, None, None, None, 1.0, None, 1, None, None, 1, 4, 0, 0, 0, 1, 0, 0, None) == -1
    assert lib.cfhip_k_sample_advance(None, None, 1, None, 0, 1, None) == -1
    assert lib.cfhip_timestep_embedding_f32(None, None, 1, 4, 10000.0, None) == -1
