"""DDIM / ancestral sampling, host side (no GPU): the noise-schedule buffers and every DDIM table equal the reference's
bit for bit (tests/golden/ddpm_samplers.pt, tools/gen_sampler_golden.py), the per-step table reproduces the reference's
step arithmetic exactly when the kernel's operation order is applied to it on the CPU, argument validation, the
reference options that are not built raise, and the C-ABI rows exist."""
import os
import re

import pytest
import torch

import cflearn_amd  # noqa: F401
from cflearn_amd import _lib, ops
from cflearn_amd.diffusion import DiffusionSampler, NoiseSchedule, ddim_tables, make_sampler, sampler_table
from sampler_replay import decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("ddpm_samplers.pt")


def _eq(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), f"{what}: max diff {(a.double() - b.double()).abs().max().item()}"


def test_schedule_posterior_buffers_bit_exact(fx):
    for sched, want in fx["tables"]["posterior"].items():
        s = NoiseSchedule(beta_schedule=sched)
        for name, v in want.items():
            _eq(getattr(s, name), v, f"{sched} {name}")


def test_ddim_tables_bit_exact(fx):
    assert len(fx["tables"]["ddim"]) == 16
    for rec in fx["tables"]["ddim"]:
        s = NoiseSchedule(beta_schedule=rec["schedule"])
        tb = ddim_tables(s, rec["steps"], rec["discretize"], rec["eta"])
        what = f"{rec['schedule']}/{rec['discretize']}/{rec['steps']}/eta {rec['eta']}"
        assert tb["timesteps"] == rec["timesteps"], what
        for name in ("alphas", "alphas_prev", "sigmas", "sqrt_one_minus_alphas"):
            _eq(tb[name], rec[name], f"{what} {name}")
    # the reference's quirk: `uniform` yields one more q-timestep than steps
    assert len(ddim_tables(NoiseSchedule(), 10)["timesteps"]) == 11


def test_step_table_reproduces_the_reference_steps(fx):
    """row k of `sampler_table` equals the scalars the reference formed for step k, and the kernel's formula over them,
    chained from z, gives every intermediate image of the reference bit for bit (SHA-256 of each)"""
    assert len(fx["steps"]) == 8
    for r in fx["steps"]:
        s = NoiseSchedule(beta_schedule=r["schedule"], parameterization=r["parameterization"])
        tb = sampler_table(r["kind"], s, r["steps"], discretize=r["discretize"], eta=r["eta"])
        _eq(tb, r["table"], f"{r['kind']} {r['parameterization']} step scalars")  # the reference's own, bit for bit
        d = decode(fx, r)  # asserts each image
        assert d["images"].shape == (r["steps"] + 1, *fx["step_z"].shape)


def test_basic_table_timesteps_and_noise_mask():
    tb = sampler_table("basic", NoiseSchedule(), 20)
    assert tb[:, 0].tolist() == [float(t) for t in range(19, -1, -1)]
    assert tb[-1, 3].item() == 0.0 and (tb[:-1, 3] > 0).all()


class _Tiny(torch.nn.Module):
    in_channels = 3

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_unbuilt_options_raise():
    u = _Tiny()
    for kind in ("plms", "k_euler", "solver", "lcm"):
        with pytest.raises(NotImplementedError):
            make_sampler(kind, u)
    with pytest.raises(NotImplementedError):
        make_sampler("ddim", u, noise_dropout=0.1)
    with pytest.raises(NotImplementedError):
        make_sampler("ddim", u, quantize_denoised=True)
    with pytest.raises(NotImplementedError):
        make_sampler("ddim", u, unconditional_cond={"concat": torch.zeros(1, 2, 3)})
    with pytest.raises(NotImplementedError):
        make_sampler("basic", u, unconditional_cond=torch.zeros(1, 2, 3), unconditional_guidance_scale=3.0)
    with pytest.raises(NotImplementedError):
        make_sampler("basic", u, NoiseSchedule(parameterization="v"))
    s = make_sampler("ddim", u)
    for kw in (dict(ref=torch.zeros(1), ref_mask=torch.zeros(1)), dict(control=[torch.zeros(1)]), dict(start_step=3),
               dict(step_callback=print)):
        with pytest.raises(NotImplementedError):
            s.sample(torch.zeros(1, 3, 4, 4), **kw)


def test_argument_validation():
    u = _Tiny()
    with pytest.raises(ValueError):
        make_sampler("nope", u)
    with pytest.raises(ValueError):
        make_sampler("ddim", u, NoiseSchedule(parameterization="x0"))
    with pytest.raises(ValueError):
        make_sampler("ddim", u, discretize="cubic")
    with pytest.raises(ValueError):
        make_sampler("ddim", u, unconditional_cond=torch.zeros(2, 3, 4))
    with pytest.raises(ValueError):
        ddim_tables(NoiseSchedule(), 0)
    with pytest.raises(ValueError):
        ddim_tables(NoiseSchedule(), 1001)
    with pytest.raises(TypeError):
        make_sampler("ddim", u, bogus=1)
    s = make_sampler("ddim", u, default_steps=7)
    assert isinstance(s, DiffusionSampler) and s.default_steps == 7 and s.eta == 0.0
    assert make_sampler("basic", u).default_steps == 1000
    with pytest.raises(TypeError):
        s.sample(torch.zeros(1, 3, 4, 4), bogus=1)
    with pytest.raises(RuntimeError):  # the UNet lives on the CPU: no eager fallback
        s.sample(torch.zeros(1, 3, 4, 4))
    # the C-ABI rejects bad arguments before any launch
    lib = _lib.load()
    assert lib.cfhip_diffusion_sample_step(None, None, None, None, 1.0, None, 1, None, None, 1, 4, 0, 0, 1.0, 0, 1, 0, 0, None) == -1
    assert lib.cfhip_randn_f32(None, 4, 0, 0, None) == -1
    assert lib.cfhip_diffusion_sample_advance(None, None, 1, None, 1, None) == -1


def test_sampler_symbols_in_header_and_signatures():
    text = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    for name in ("cfhip_randn_f32", "cfhip_diffusion_sample_step", "cfhip_diffusion_sample_advance"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    assert f"#define CFHIP_SAMPLE_ROW {ops.SAMPLE_ROW}" in text
