"""Image-to-image and inpainting sampling, host side (no GPU): the side table and the `start_step` tables against the reference's
scalars (tests/golden/img2img_samplers.pt, tools/gen_img2img_golden.py), `DiffusionAPI._q_sample`'s grid, the kernel's documented
operation order in numpy f32 reproducing every recorded image of every step record, the argument checks, the Philox counter
ranges of a run and the C-ABI rows."""
import os
import re

import numpy as np
import pytest
import torch

import cflearn_amd  # noqa: F401
from cflearn_amd import _lib, ops
from cflearn_amd.diffusion import (K_COLUMNS, NoiseSchedule, _q_weights, k_sampler_table, k_sigma_tables, make_sampler,
                                   sampler_philox_ranges, sampler_side_table, sampler_table)
from img2img_replay import K_KINDS, decode, merge_formula, record_id
from k_sampler_replay import COL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ddim", "basic") + K_KINDS
# as tests/test_k_sampler_host.py: columns that pass through log / exp / pow / expm1 may differ by 1 f32 ulp between math libraries
ULP_COLUMNS = ("t", "expm1_neg_h", "r_plus", "r_minus")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("img2img_samplers.pt")


def _eq(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a, b), f"{what}: max diff {(a.double() - b.double()).abs().max().item()}"


def _within_one_ulp(a, b, what):
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    ulp = torch.ldexp(torch.ones_like(b), (torch.frexp(b.abs().clamp_min(2.0 ** -126))[1] - 24).to(torch.int32))
    bad = (a - b).abs() > ulp
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} entries beyond 1 ulp, e.g. {a[bad][:3].tolist()} vs {b[bad][:3].tolist()}"


def test_fixture_covers_the_grid(fx):
    """five kinds x start_step {0, 3} x {no reference, both mask layouts} x guidance {off, 7.5} x eps and v / x0; per-merge and
    unified noise for ddim / basic; masks with 0, 1 and fractional values; H W = 9"""
    assert tuple(fx["step_z"].shape) == (2, 4, 3, 3) and tuple(fx["k_columns"]) == K_COLUMNS == tuple(COL)
    assert tuple(fx["step_masks"]["b1"].shape) == (2, 1, 3, 3) and tuple(fx["step_masks"]["1c"].shape) == (1, 4, 3, 3)
    for m in fx["step_masks"].values():
        assert bool((m == 0).any()) and bool((m == 1).any()) and bool(((m > 0) & (m < 1)).any())
    seen = {(r["kind"], r["parameterization"], r["start_step"], r["mask"], r["scale"] is not None) for r in fx["steps"]}
    pars = {"ddim": ("eps", "v"), "basic": ("eps", "x0"), **{k: ("eps", "v") for k in K_KINDS}}
    want = {(k, p, s, m, g) for k in KINDS for p in pars[k] for s in (0, 3) for m in (None, "b1", "1c") for g in (False, True)}
    assert seen == want and len(fx["steps"]) == len(want) == 120
    for r in fx["steps"]:
        assert r["unified"] == (r["kind"] in ("ddim", "basic") and r["mask"] == "1c")


def test_numpy_replica_reproduces_every_reference_image(fx):
    """the kernel's operation order — merge in front of every ddim / basic step, merged `denoised` inside every K evaluation, the
    state taken as it stands when the run starts part-way — rebuilds the image after every step of every record (decode asserts
    each SHA-256): the order of operations is pinned to the reference on the CPU"""
    for r in fx["steps"]:
        d = decode(fx, r)
        assert len(d["images"]) == r["steps"] - r["start_step"] + 1
        if r["kind"] in K_KINDS:
            assert np.array_equal(d["images"][-1], d["images"][-2])  # the last step returns the image as it is
            if r["mask"] is not None:  # where the mask is exactly 1 every merged denoised IS the reference
                keep = np.broadcast_to(d["mask"] == 1, d["ref"].shape)
                assert keep.any() and all(np.array_equal(den[keep], d["ref"][keep]) for den in d["denoised"])


def test_side_and_step_tables_equal_the_reference_scalars(fx):
    for r in fx["steps"]:
        s = NoiseSchedule(beta_schedule=r["schedule"], parameterization=r["parameterization"])
        what, start = record_id(r), r["start_step"]
        if r["kind"] not in K_KINDS:
            tb = sampler_table(r["kind"], s, r["steps"], discretize=r["discretize"], eta=r["eta"])
            _eq(tb[start:], r["table"], f"{what} step scalars")  # the full run's rows: the counter is absolute
            side = sampler_side_table(r["kind"], s, r["steps"], discretize=r["discretize"])
            assert side.shape == (r["steps"], 2)
            _eq(side[start:], r["side"], f"{what} side table")  # sqrt is correctly rounded: bit for bit
            continue
        tb = k_sampler_table(r["kind"], s, r["steps"], sigmas_scheduler=r["sigmas_scheduler"], quantize=r["quantize"], start_step=start)
        assert tuple(tb.shape) == tuple(r["table"].shape)
        _within_one_ulp(tb[:, COL["sigma"]], r["table"][:, COL["sigma"]], f"{what} sigma")
        same_sigma = torch.equal(tb[:, COL["sigma"]], r["table"][:, COL["sigma"]])
        for name, i in COL.items():
            if name in ULP_COLUMNS and not (name == "t" and r["quantize"]):
                _within_one_ulp(tb[:, i], r["table"][:, i], f"{what} {name}")
            elif name != "sigma" and same_sigma:
                _eq(tb[:, i], r["table"][:, i], f"{what} {name}")
        if r["kind"] == "k_dpmpp_2m":  # the first EXECUTED row has no old_denoised
            flags = tb[:, COL["flag"]].tolist()
            assert flags == [0.0 if e in (0, start) else 1.0 for e in range(r["steps"] - 1)]
            assert tb[start, COL["r_plus"]].item() == 0.0 and tb[start, COL["r_minus"]].item() == 0.0


def test_start_step_leaves_the_other_rows_alone():
    s = NoiseSchedule()
    for kind in K_KINDS:
        full = k_sampler_table(kind, s, 9)
        part = k_sampler_table(kind, s, 9, start_step=4)
        differ = (full != part).any(dim=1).nonzero().flatten().tolist()
        assert differ == ([4] if kind == "k_dpmpp_2m" else [])


def test_q_sample_grid(fx):
    """`DiffusionAPI._q_sample` (called by the generator with a stand-in `self`): (t, start_step) per family, and the q-sampled z.
    K: t = min(n, round((1 - f)(n + 1))) - 1, start = n - t - 1, so f = 0.5 gives round(4.5) = 4 -> (3, 4) at n = 8 and
    round(5.5) = 6 -> (5, 4) at n = 10 (Python rounds ties to even); others: t = int(min(1 - f, 0.999) n), start = n - t, so
    f = 0 gives t = int(0.999 * 8) = 7, start 1, and f = 1 starts at n (nothing runs).
    ddim / basic z: correctly rounded operations on bit-equal tables, so bit for bit.  K z = z_ref + sigma * noise with sigma
    within 1 ulp (exp): |noise| < 4 and sigma < 16 (ulp 2^-20) move the product by < 2^-18, and the product's and the sum's own
    roundings (|values| < 64: half an ulp of 2^-18 each) add up to less than 2^-16."""
    u = _Tiny()
    points = {(q["fidelity"], q["num_steps"]) for q in fx["q_sample"]}
    assert {(0.0, 8), (1.0, 8), (0.999, 8), (0.5, 8), (0.5, 10)} <= points
    qz, qn = fx["q_z"], fx["q_noise"]
    worked = {("k_euler_a", 0.5, 8): (3, 4), ("k_euler_a", 0.5, 10): (5, 4), ("k_euler_a", 0.0, 8): (7, 0), ("k_euler_a", 1.0, 8): (-1, 8),
              ("ddim", 0.0, 8): (7, 1), ("ddim", 1.0, 8): (0, 8), ("basic", 0.999, 8): (0, 8), ("ddim", 0.5, 8): (4, 4)}
    for q in fx["q_sample"]:
        s = make_sampler(q["kind"], u)
        t, start = s.img2img_start(q["fidelity"], q["num_steps"])
        assert (t, start) == (q["t"], q["start_step"]), (q["kind"], q["fidelity"], q["num_steps"])
        key = (q["kind"], q["fidelity"], q["num_steps"])
        if key in worked:
            assert (t, start) == worked[key], key
        if q["kind"] in K_KINDS:
            sigmas = k_sigma_tables(s.schedule, q["num_steps"])["sigmas"]
            z = qz + sigmas[start] * qn
            assert (z - q["z"]).abs().max().item() < 2.0 ** -16, key
            if start == q["num_steps"]:
                _eq(z, qz, "fidelity 1 keeps the reference")
        else:
            w_net, w_noise = _q_weights(q["kind"], s.schedule, q["num_steps"])
            _eq(w_net[t] * qz + w_noise[t] * qn, q["z"], f"{key} z")


def test_merge_formula_is_the_documented_expression():
    rng = np.random.default_rng(0)
    x, ref, nz = (rng.standard_normal((2, 4, 3, 3)).astype(np.float32) for _ in range(3))
    mask = rng.random((2, 1, 3, 3)).astype(np.float32)
    a, b = np.float32(0.8), np.float32(0.6)
    y = merge_formula(x, ref, mask, a, b, nz)
    for i in np.ndindex(*x.shape):
        m = mask[i[0], 0, i[2], i[3]]
        want = np.float32(m * np.float32(np.float32(a * ref[i]) + np.float32(b * nz[i]))) + np.float32(np.float32(np.float32(1) - m) * x[i])
        assert y[i] == np.float32(want)
    ones, zeros = np.ones_like(mask), np.zeros_like(mask)
    assert np.array_equal(merge_formula(x, ref, zeros, a, b, nz), x)
    assert np.array_equal(merge_formula(x, ref, ones, a, b, nz), a * ref + b * nz)


class _Tiny(torch.nn.Module):
    in_channels = 4

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_argument_validation():
    """everything is refused on the host, before the device is asked for (the UNet here lives on the CPU: a call that passes
    the checks ends in the RuntimeError of the device test)"""
    u = _Tiny()
    z, ref = torch.zeros(2, 4, 3, 3), torch.zeros(2, 4, 3, 3)
    good_masks = [torch.zeros(2, 1, 3, 3), torch.zeros(1, 4, 3, 3), torch.zeros(1, 1, 3, 3), torch.zeros(2, 4, 3, 3)]
    for kind in KINDS:
        s = make_sampler(kind, u)
        for kw in (dict(ref=ref, ref_mask=good_masks[0]), dict(start_step=3), dict(step_callback=print)):  # `sample` still refuses
            with pytest.raises(NotImplementedError):
                s.sample(z, **kw)
        with pytest.raises(NotImplementedError, match="sample_with_reference"):
            s.sample(z, ref=ref, ref_mask=good_masks[0])
        with pytest.raises(NotImplementedError, match="sample_with_reference"):
            s.sample(z, start_step=2)
        run = lambda **kw: s.sample_with_reference(z, num_steps=8, **kw)  # noqa: E731
        with pytest.raises(ValueError, match="go together"):
            run(ref_mask=good_masks[0])  # a mask without a ref
        with pytest.raises(ValueError, match="go together"):
            run(ref=ref)
        for bad in (torch.zeros(2, 4, 3, 4), torch.zeros(1, 4, 3, 3), torch.zeros(2, 4, 9)):
            with pytest.raises(ValueError, match="`ref` must"):
                run(ref=bad, ref_mask=good_masks[0])
        for bad in (torch.zeros(2, 2, 3, 3), torch.zeros(3, 1, 3, 3), torch.zeros(2, 1, 3, 4), torch.zeros(2, 3, 3)):
            with pytest.raises(ValueError, match="`ref_mask` must"):
                run(ref=ref, ref_mask=bad)
        for bad in (-1, 9):
            with pytest.raises(ValueError, match="start_step"):
                run(start_step=bad)
        with pytest.raises(ValueError, match="need a reference"):
            run(use_unified_ref_noise=True, ref_noise=ref)
        with pytest.raises(NotImplementedError):
            run(step_callback=print)
        with pytest.raises(TypeError):
            run(bogus=1)
        with pytest.raises(NotImplementedError):
            run(cond={"concat": torch.zeros(1)}, ref=ref, ref_mask=good_masks[0])
        if kind in K_KINDS:  # the K samplers merge without noise: every reference-noise option is refused
            for kw in (dict(ref_noise=ref), dict(use_unified_ref_noise=True, ref_noise=ref), dict(ref_noise_bank=torch.zeros(8, 2, 4, 3, 3))):
                with pytest.raises(ValueError, match="without noise"):
                    run(ref=ref, ref_mask=good_masks[0], **kw)
        else:
            with pytest.raises(ValueError, match="needs `ref_noise`"):
                run(ref=ref, ref_mask=good_masks[0], use_unified_ref_noise=True)
            with pytest.raises(ValueError, match="`ref_noise` must"):
                run(ref=ref, ref_mask=good_masks[0], use_unified_ref_noise=True, ref_noise=torch.zeros(2, 4, 3, 4))
            for bad, start in ((torch.zeros(7, 2, 4, 3, 3), 0), (torch.zeros(8, 2, 4, 3, 3), 3), (torch.zeros(8, 2, 4, 3, 4), 0)):
                with pytest.raises(ValueError, match="ref_noise_bank"):
                    run(ref=ref, ref_mask=good_masks[0], ref_noise_bank=bad, start_step=start)
            with pytest.raises(ValueError, match="not both"):
                run(ref=ref, ref_mask=good_masks[0], ref_noise_bank=torch.zeros(8, 2, 4, 3, 3), use_unified_ref_noise=True, ref_noise=ref)
        for m in good_masks:  # well-formed operands pass every check and reach the device test
            with pytest.raises(RuntimeError, match="HIP device"):
                run(ref=ref, ref_mask=m, start_step=3)
        with pytest.raises(RuntimeError, match="HIP device"):
            s.img2img(ref, fidelity=0.5, num_steps=8)
        with pytest.raises(RuntimeError, match="HIP device"):
            s.inpaint(ref, good_masks[0], num_steps=8)
    for kind in ("plms", "klms", "k_euler", "k_dpmpp_2m_sde", "solver", "lcm"):
        with pytest.raises(NotImplementedError):
            make_sampler(kind, u)
    for kw in (dict(noise_dropout=0.1), dict(quantize_denoised=True)):
        with pytest.raises(NotImplementedError):
            make_sampler("ddim", u, **kw)


def test_philox_counter_ranges_of_a_run_are_disjoint():
    """the starting noise, the draw of every row and the noise of every merge of one (seed, offset) never share a counter"""
    for total, rows, row0 in ((72, 8, 0), (72, 8, 3), (4, 1, 0), (2 * 4 * 64 * 64, 50, 17)):
        r = sampler_philox_ranges(total, rows, row0)
        spans = [r["start"], *r["steps"].values(), *r["merges"].values()]
        assert len(spans) == 1 + 2 * (rows - row0)
        assert all(hi - lo == total // 4 for lo, hi in spans)
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (total, rows, row0)
        assert r["start"] == (0, total // 4) and r["steps"][row0][0] == (1 + row0) * (total // 4)
        assert r["merges"][row0][0] == (1 + rows + row0) * (total // 4)
        # a part-way run draws what the full run draws at the same rows
        full = sampler_philox_ranges(total, rows, 0)
        assert all(full["steps"][k] == v for k, v in r["steps"].items()) and all(full["merges"][k] == v for k, v in r["merges"].items())


def test_symbols_constants_and_null_arguments():
    text = open(os.path.join(ROOT, "include", "cfhip.h")).read()
    for name in ("cfhip_diffusion_sample_step_ref", "cfhip_diffusion_sample_merge", "cfhip_k_sample_step_ref"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    assert ops.MERGE_NOISE == {"philox": 0, "unified": 1, "bank": 2}
    assert ops.SAMPLE_ROW == 8 and ops.KSAMPLE_ROW == 12  # the existing rows keep their width
    # the existing entry points keep their signatures: the new operands ride behind them
    old, new = _lib.SIGNATURES["cfhip_diffusion_sample_step"], _lib.SIGNATURES["cfhip_diffusion_sample_step_ref"]
    assert new[1][:len(old[1]) - 1] == old[1][:-1] and len(new[1]) == len(old[1]) + 9
    old, new = _lib.SIGNATURES["cfhip_k_sample_step"], _lib.SIGNATURES["cfhip_k_sample_step_ref"]
    assert new[1][:len(old[1]) - 1] == old[1][:-1] and len(new[1]) == len(old[1]) + 5
    lib = _lib.load()  # null arguments are rejected with -1 before any launch
    assert lib.cfhip_diffusion_sample_step_ref(None, None, None, None, 1.0, None, 1, None, None, 1, 4, 0, 0, 1.0, 0, 1, 0, 0,
                                               None, None, 0, 0, 4, None, None, 0, 0, None) == -1
    assert lib.cfhip_diffusion_sample_merge(None, None, 1, None, 1, 4, 1, 0, 0, None, None, 0, 0, 4, None, None, 0, 0, None) == -1
    assert lib.cfhip_k_sample_step_ref(None, None, None, None, None, 1.0, None, 1, None, None, 1, 4, 0, 0, 0, 1, 0, 0,
                                       None, None, 0, 0, 4, None) == -1
